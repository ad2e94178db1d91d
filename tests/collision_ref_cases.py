"""Cases shared by tests/test_collision_ref_host.py and tests/test_gpu_collision_ref.py: the
probe fixtures, and a fixed subset of pair_hulls.pose_sets with the independent reference's
depth (collision_ref.depth over the fixture's link vertices) of every pair, computed once.

The oracle only places the poses (pose_sets moves a link along a line until the oracle's depth
is 0.04 + d); what the tests compare with is the reference depth of those poses."""
import functools
import os

import numpy as np

import collision_ref as C

P = 0.04
SIDE = 0.99e-7  # a pair at least this far from P has a side every implementation must take
HERE = os.path.dirname(os.path.abspath(__file__))

N_BOX_NEAR, N_BOX_FREE = 260, 40
N_MESH_NEAR, N_MESH_FREE = 80, 20
# every library shape once, the three scales in turn
LIBRARY_PICK = (0, 4, 8, 9, 13, 17, 18, 22, 26)


@functools.lru_cache(maxsize=None)
def probes():
    z = np.load(os.path.join(HERE, "golden", "collision_probes.npz"))
    return {k: z[k] for k in z.files}


def pose_vertices(link, pose12):
    """World vertices of moving link `link` (the fixture's mesh) at a frame row of 12."""
    pose12 = np.asarray(pose12, dtype=np.float64)
    return C.link_vertices(C.LINKS[link]) @ pose12[:9].reshape(3, 3).T + pose12[9:]


def box_mesh(row):
    """An obstacle box row as an 8-vertex ConvexMesh (the hull-vs-hull path's input)."""
    from torque_constrained_motion_planning_amd.hull import ConvexMesh
    return ConvexMesh(C.box_vertices(row), name="box as mesh")


class HullPack:
    """The exact hulls and boxes of tcmp_set_meshes alone, no LODs and no spheres (both are
    optional accelerations): what Engine.set_scene needs of a hull.MeshPack, at a tenth of the
    packing time, for tests that install hundreds of one-mesh scenes."""

    def __init__(self, vertex_sets):
        from torque_constrained_motion_planning_amd.hull import HullSet, fit_boxes, hull_data
        recs = [hull_data(np.asarray(v, dtype=np.float64)) for v in vertex_sets]
        hs = HullSet(recs)
        self.__dict__.update(hs.__dict__)
        self._arrays = hs.arrays()
        self.n = len(recs)
        self.boxes = np.ascontiguousarray(np.array(
            [np.concatenate([c, R.reshape(-1), half, ih])
             for c, R, half, ih in (fit_boxes(r[0], r[1]) for r in recs)]).reshape(-1, 18))
        self.inner = self.spheres = None

    def key(self):
        return b"hulls only" + b"".join(a.tobytes() for a in self._arrays + (self.boxes,))

    def __len__(self):
        return self.n


def _pick(ps, n_near_per_link, rng, prefer=None):
    """n_near_per_link poses of every link, the offset classes taken in turn so that all twelve
    occur; `prefer` (obstacle ids) wins every third pick where it has a candidate."""
    import pair_hulls as PH
    out = []
    for link in range(10):
        for j in range(n_near_per_link):
            d = PH.OFFSETS[(link * n_near_per_link + j) % len(PH.OFFSETS)]
            cand = np.flatnonzero((ps.link == link) & (ps.offset == d))
            assert len(cand), (link, d)
            if prefer is not None and j % 3 == 0:
                pc = cand[np.isin(ps.obstacle[cand], prefer)]
                cand = pc if len(pc) else cand
            out.append(int(rng.choice(cand)))
    return np.array(out)


class PoseCases:
    """meshes / pack / boxes: the obstacles; box, mesh: PoseSets (300 and 100 pairs); box_ref,
    mesh_ref: the reference depth of each pair."""

    def __init__(self):
        import oracle as O
        import pair_hulls as PH
        from torque_constrained_motion_planning_amd.hull import pack_meshes
        lib = PH.library_meshes()
        self.meshes = [lib[i] for i in LIBRARY_PICK] + PH.degenerate_meshes()
        self.degenerate = np.arange(len(LIBRARY_PICK), len(self.meshes))
        self.pack = pack_meshes(self.meshes)
        self.boxes = PH.box_obstacles()
        pk = self.pack
        self.mesh_verts = [pk.verts[pk.vert_off[m]:pk.vert_off[m + 1]] for m in range(len(pk))]
        cen = np.array([v.mean(0) for v in self.mesh_verts])
        O.set_meshes(self.pack)
        try:
            near, free, _ = PH.pose_sets(lambda l, f, o: O.pair_pd_pose_batch(l, f, o, 1), cen,
                                         seed=303, n_free=N_MESH_FREE)
        finally:
            O.set_meshes(None)
        rng = np.random.default_rng(77)
        self.mesh = PH.PoseSet.concat([near.take(_pick(near, N_MESH_NEAR // 10, rng,
                                                       self.degenerate)), free])
        near, free, _ = PH.pose_sets(
            lambda l, f, o: O.pair_pd_pose_batch(l, f, o, 1, self.boxes), self.boxes[:, :3],
            seed=404, n_free=N_BOX_FREE)
        self.box = PH.PoseSet.concat([near.take(_pick(near, N_BOX_NEAR // 10, rng)), free])
        assert len(self.box) == 300 and len(self.mesh) == 100
        assert set(self.degenerate) <= set(self.mesh.obstacle)
        for ps in (self.box, self.mesh):
            assert set(ps.link) == set(range(10))
            assert set(ps.offset[~np.isnan(ps.offset)]) == set(PH.OFFSETS)
        box_v = [C.box_vertices(b) for b in self.boxes]
        self.box_ref = np.array([C.depth(pose_vertices(l, f), box_v[o])
                                 for l, f, o in zip(self.box.link, self.box.pose, self.box.obstacle)])
        self.mesh_ref = np.array([C.depth(pose_vertices(l, f), self.mesh_verts[o])
                                  for l, f, o in zip(self.mesh.link, self.mesh.pose,
                                                     self.mesh.obstacle)])


@functools.lru_cache(maxsize=None)
def pose_cases():
    return PoseCases()
