"""Writes tests/golden/attach_cases.npz: what the restatement (tests/attach_ref.py over
tests/collision_ref.py, the oracle's arm-and-torque walk) says of the cases of
tests/attach_cases.py.  Run from the repository root after the oracle is built:
python tests/golden/gen_attach_cases.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")]

import attach_cases as K  # noqa: E402

out = {}
out.update(K.build_depths())
out.update(K.build_flags())
out.update(K.build_edges())
out.update(K.build_small())
np.savez_compressed(K.RECORD, **out)
print("wrote %s: %s" % (K.RECORD, {k: v.shape for k, v in out.items()}))
