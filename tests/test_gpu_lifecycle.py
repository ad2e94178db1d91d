"""An engine gives back what it took: create / use / close cycles in one process.

A cycle creates an engine on device 0, sets a 4-box scene, grows and finishes a small plan
(2,048 samples, batch 256, trajectory finish), calls one stand-alone `retime`, `collides` and
`rne` on 64 rows -- so the plan's buffers, the index, the finish's pinned staging, `rt_*`, `s*`
and `i*` are all allocated -- and closes it.  After a warm-up cycle, eight cycles run; the
device's free memory is read after every close.

The reading is `hipMemGetInfo` of the HIP runtime the engine's library is linked against, looked
up through the library's own handle.  `torch.cuda.mem_get_info(0)` reads the same device-wide
figure and worked in a process of its own, but torch brings a second HIP runtime in its wheel,
and that one finds no GPU once the engine's runtime has initialised the device -- which, in the
whole suite, earlier test modules have done long before this one runs.

* Free memory after cycle 8 is no lower than after cycle 1 by more than F / 2, F being one live
  engine's footprint (free memory before `Engine(0)` minus free memory just before `close()`).
  F = FOOTPRINT below was measured with this very cycle on the parent commit cfe686d's library
  on an MI355X, the same in each of its eight cycles: 12,582,912 bytes read through
  `torch.cuda.mem_get_info` and 18,874,368 through this test's own reading (the test prints the
  footprint it sees each run); the constant is the smaller, so the stricter, of the two.  A
  handle that kept its buffers would lose about 7 F over the eight cycles; F / 2 absorbs the
  allocator's granularity.  Two idle reads a second apart did not differ (five pairs).
* Every cycle's plan -- every field of the result but the timings, and the fetched waypoints and
  trajectory rows -- equals cycle 1's byte for byte.

What this does not catch: a leak far below the allocator's granularity.  The shared-tree
rounds' exchange slots (`xch`, a few words), which `tcmp_destroy` used to forget, are of that
size, and so are events.  That nothing of the kind is left behind follows from the handle's
members owning their resources (csrc/tcmp_engine.hip), not from this test.  The
reading is device-wide, so another process's allocations on the same device move it too.
"""
import ctypes

import numpy as np
import pytest

import oracle as O  # noqa: E402  (test infrastructure)

pytestmark = pytest.mark.gpu

FOOTPRINT = 12582912  # bytes; see the docstring
CYCLES = 8
N_SAMPLES, BATCH, SEED = 2048, 256, 7
START = np.array([0, -np.pi / 4, 0.0, -6 * np.pi / 8, 0, np.pi / 2, np.pi / 4])
GOAL = np.array([0.5, 0.2, 0.1, -1.5, 0.3, 1.8, 0.2])


def _plan_record(r, rows):
    skip = lambda f: f == "ms" or f.startswith("ms_")  # noqa: E731
    fields = tuple((f, getattr(r, f)) for f, _ in r._fields_ if not skip(f))
    return repr(fields).encode() + b"".join(
        k.encode() + repr(rows[k].shape).encode() + rows[k].tobytes() for k in sorted(rows))


def _cycle(_lib, obs, free_mem):
    before = free_mem()
    e = _lib.Engine(0)
    try:
        e.set_scene(obs)
        assert e.plan_begin(START, GOAL, _lib.TORQUE_RNE, 5.0, 1.0, max_nodes=N_SAMPLES + 1,
                            max_batch=BATCH, seed=SEED) == _lib.PLAN_OK
        e.plan_run(N_SAMPLES, BATCH)
        r = e.plan_finish()
        rows = e.plan_fetch(r)
        assert r.n_traj > 0  # a trajectory finish: the rows and their pinned staging exist
        rec = _plan_record(r, rows)
        rng = np.random.default_rng(3)
        q = rng.uniform(-1.5, 1.5, (64, 7))
        v = rng.uniform(-0.5, 0.5, (64, 7))
        a = rng.uniform(-2.0, 2.0, (64, 7))
        e.retime(q, v, a, _lib.TORQUE_RNE, 5.0)
        e.collides(q)
        e.rne(q, v, a, 5.0)
        footprint = before - free_mem()
    finally:
        e.close()
    return rec, footprint, free_mem()


def test_cycles_return_their_memory_and_repeat_their_plan():
    from torque_constrained_motion_planning_amd import _lib
    from torque_constrained_motion_planning_amd.scene import obstacle_array, random_box_scene

    mem_get_info = _lib.load_library().hipMemGetInfo  # (dlsym searches its dependencies)

    def free_mem():
        free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert mem_get_info(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    obs = obstacle_array(random_box_scene(np.random.default_rng(0), 4, avoid=[START, GOAL],
                                          collides=lambda q, o: O.collision(q, o)))
    assert len(obs) == 4
    free_mem()
    _cycle(_lib, obs, free_mem)  # warm-up: the runtime's own one-time allocations
    recs, free_after = [], []
    for c in range(CYCLES):
        rec, footprint, free = _cycle(_lib, obs, free_mem)
        print("cycle %d: footprint %d bytes, free after close %d" % (c + 1, footprint, free))
        recs.append(rec)
        free_after.append(free)
    print("free after cycle 1 minus after cycle %d: %d bytes (allowed: %d)"
          % (CYCLES, free_after[0] - free_after[-1], FOOTPRINT // 2))
    for c in range(1, CYCLES):
        assert recs[c] == recs[0], "cycle %d's plan differs from cycle 1's" % (c + 1)
    assert free_after[0] - free_after[-1] <= FOOTPRINT // 2
