"""rm_sdf_mesh's definition without a GPU.  First the NumPy specification (tests/sdf_mesh_spec.py) against geometry, on lattices of
the oracle's sdScene: a definition that orders a quad the wrong way round, drops one, or places a vertex outside its cell fails here.
Then the library's own per-cell and per-edge functions (raymarcher_amd/csrc/rm_surface_nets.h, the code the kernels call), run
serially by a stand-alone CPU program under the address and undefined-behaviour sanitizers, against that specification in every bit
— which pins the device code's arithmetic before any GPU run."""
import numpy as np
import pytest

import sdf_helpers as V
import sdf_mesh_spec as S

SPHERE = ("sphere", (12, 12, 12))
SPHERE_CUBE = ("sphere_cube", (21, 11, 11))


def _mesh(name, dims, iso=0.0):
    dist, ids, origin, step = V.oracle_lattice(name, dims)
    return S.surface_nets(dist, origin, step, iso, ids), dist, origin, step


def test_lattice_points_are_one_multiply_and_one_add():
    origin, step, dims = np.array([0.1, -0.7, 3.0], np.float32), np.array([0.3, 0.01, 1e-3], np.float32), (5, 7, 9)
    pts = S.lattice_points(origin, step, dims)
    assert pts.shape == (5 * 7 * 9, 3) and pts.dtype == np.float32
    for q in (0, 1, 5, 34, 35, 314):
        i, j, k = q % 5, (q // 5) % 7, q // 35
        want = [np.float32(origin[a] + np.float32(np.float32(n) * step[a])) for a, n in enumerate((i, j, k))]
        assert [x.tobytes() for x in pts[q]] == [x.tobytes() for x in want], q
    # fused, 0.1 + 3 · 0.3 would round differently for at least one of these: the products are rounded first
    assert pts[3, 0] == np.float32(np.float32(3) * np.float32(0.3)) + np.float32(0.1)


def test_unit_sphere_is_closed_oriented_and_its_volume_is_the_lattices():
    """The lattice spans [−0.8, 0.8]³ around a sphere of radius 0.5: the surface is strictly inside.  Volume bound, from the
    construction alone: a cell that is not active has all corners inside or all outside, the mesh's surface lies in active cells only
    (every vertex in its own cell, every quad over four active cells around their common edge), and so does the boundary of the
    union of the cubes of one step around the inside lattice points, of which the mesh is a deformation.  Both solids hold every
    all-inside cell and no all-outside one, so both volumes lie between the all-inside cells' volume and that plus the active cells'
    volume: they differ by less than the active cells' volume."""
    m, dist, origin, step = _mesh(*SPHERE)
    v, q = m["vertices"], m["quads"]
    assert len(v) > 50 and len(q) > 50
    edges = V.assert_closed_oriented(q, "sphere")
    assert len(v) - edges + len(q) == 2
    assert (np.unique(q) == np.arange(len(v))).all(), "a vertex no quad uses"
    cell_volume = float(np.prod(step.astype(np.float64)))
    volume = V.signed_volume(v, q)
    assert volume > 0
    inside_points = int((dist < 0).sum())
    assert abs(volume - inside_points * cell_volume) < len(v) * cell_volume
    # every vertex lies inside its own cell
    axes = S.lattice_axes(origin, step, SPHERE[1])
    for a in range(3):
        lo, hi = axes[a][m["cells"][:, a]], axes[a][m["cells"][:, a] + 1]
        assert ((v[:, a] >= lo) & (v[:, a] <= hi)).all(), f"axis {a}"
    assert (v[:, 3] == 0).all()
    # and close to the sphere: within a cell's diagonal of radius 0.5
    r = np.linalg.norm(v[:, :3].astype(np.float64), axis=1)
    assert np.abs(r - 0.5).max() < float(np.linalg.norm(step))


def test_sphere_and_cube_are_two_closed_components_with_their_own_ids():
    m, dist, origin, step = _mesh(*SPHERE_CUBE)
    v, q, vo = m["vertices"], m["quads"], m["vertex_object"]
    V.assert_closed_oriented(q, "sphere + cube")
    label = V.components(len(v), q)
    names = np.unique(label)
    assert len(names) == 2
    assert set(np.unique(vo)) == {0, 1}
    for comp in names:
        mine = label == comp
        qm = q[mine[q[:, 0]]]
        assert mine[qm].all()
        renumber = np.cumsum(mine) - 1
        e = V.assert_closed_oriented(renumber[qm], f"component {comp}")
        assert int(mine.sum()) - e + len(qm) == 2
        assert len(np.unique(vo[mine])) == 1, "a component with vertices of both objects"
        assert V.signed_volume(v, qm) > 0
    # the sphere (object 0) is the component on the −x side
    assert (v[vo == 0, 0] < 0).all() and (v[vo == 1, 0] > 0).all()


def test_spec_on_degenerate_lattices():
    hm = V.handmade()
    for name in ("all_inside_4x4x4", "all_outside_3x5x4", "face_only_4x4x4"):
        dist, ids, origin, step, iso = hm[name]
        m = S.surface_nets(dist, origin, step, iso, ids)
        if name == "face_only_4x4x4":  # the 3 × 3 cells along the face are active; of the 16 crossed z-edges 2 × 2 are interior in x and y
            assert len(m["vertices"]) == 9 and len(m["quads"]) == 4
        else:
            assert len(m["vertices"]) == 0 and len(m["quads"]) == 0
    dist, ids, origin, step, iso = hm["touches_boundary_3x5x4"]
    m = S.surface_nets(dist, origin, step, iso, ids)
    # two sheets of 2 × 4 cells each; only edges interior in x and y give quads: 1 × 3 per sheet
    assert len(m["vertices"]) == 16 and len(m["quads"]) == 6
    dist, ids, origin, step, iso = hm["infinities_4x4x4"]
    m = S.surface_nets(dist, origin, step, iso, ids)
    assert np.isfinite(m["vertices"]).all() and len(m["vertices"]) == 26 and len(m["quads"]) == 24
    V.assert_closed_oriented(m["quads"], "the cube of infinities")
    for d in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (1, 1, 1)):
        m = S.surface_nets(np.zeros(d[::-1], np.float32) - 1, origin, step, 0.0)
        assert len(m["vertices"]) == 0 and len(m["quads"]) == 0


@pytest.fixture(scope="module")
def cpu_program(tmp_path_factory):
    return V.build_cpu_program(tmp_path_factory.mktemp("sdf_mesh_cpu"))


ORACLE_CASES = {"sphere": (SPHERE, True, 0.0), "sphere_iso": (SPHERE, False, 0.07), "sphere_cube": (SPHERE_CUBE, True, 0.0),
                "sphere_cube_iso": (SPHERE_CUBE, False, 0.07)}
THIN_CASES = {"thin_1x4x4": (1, 4, 4), "thin_4x4x1": (4, 4, 1)}
CASE_NAMES = sorted(list(ORACLE_CASES) + list(THIN_CASES) + list(V.handmade()))


def _case(name):
    if name in ORACLE_CASES:
        (scene, dims), with_ids, iso = ORACLE_CASES[name]
        dist, ids, origin, step = V.oracle_lattice(scene, dims)
        return dist, ids if with_ids else None, origin, step, iso
    if name in THIN_CASES:
        d = THIN_CASES[name]
        return np.zeros(d[::-1], np.float32) - 1, None, np.zeros(3, np.float32), np.ones(3, np.float32), 0.0
    return V.handmade()[name]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_shared_header_on_the_cpu_equals_the_spec_in_every_bit(cpu_program, tmp_path, name):
    dist, ids, origin, step, iso = _case(name)
    want = S.surface_nets(dist, origin, step, iso, ids)
    got = V.run_cpu_program(cpu_program, tmp_path, dist, ids, origin, step, iso)
    assert len(got["vertices"]) == len(want["vertices"]) and len(got["quads"]) == len(want["quads"]), name
    V.assert_bits(got["vertices"], want["vertices"], f"{name}: vertices")
    assert (got["vertex_object"] == want["vertex_object"]).all(), f"{name}: vertex ids"
    assert (got["quads"] == want["quads"]).all(), f"{name}: quads"
