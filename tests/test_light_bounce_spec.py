"""The term of rm_shade_rays_indirect without a GPU: the library's own arithmetic behind the hit (raymarcher_amd/csrc/rm_indirect.h
over rm_light_grid.h, compiled into a stand-alone program under the address and undefined-behaviour sanitizers and run as a program)
against the NumPy definition (tests/light_bounce_spec.py) in every word on the GPU tests' grids; and properties of the definition:
an irradiance that is not positive, a NaN and a record of no probe change nothing, and the palette has its three forms."""
import numpy as np
import pytest

import light_bounce_helpers as M
import light_bounce_spec as B
import light_depth_helpers as MD
import light_grid_helpers as MG
import light_grid_spec as G

f32 = np.float32


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("light_bounce_cpu")
    return M.build_cpu_program(d), d


@pytest.mark.parametrize("with_depth", [False, True])
@pytest.mark.parametrize("facing", [False, True])
@pytest.mark.parametrize("name", list(MG.GRIDS))
def test_the_header_equals_the_definition(program, name, facing, with_depth):
    dims, origin, step, _, _ = MG.GRIDS[name]
    rec = MG.records(name)
    depth = MD.depth_records(name) if with_depth else None
    changed = 0
    for n in M.COUNTS:
        pts, nrm = MG.points(name, n)
        colour, dif, c, palette, has_term = M.ray_inputs(name, n)
        for bias in M.BIASES if with_depth else M.BIASES[:1]:
            for strength in M.STRENGTHS:
                k = B.scale_of(strength)
                light = B.grid_e(rec, depth, dims, origin, step, pts, nrm, facing, bias)
                want = B.term(colour, has_term, light["probes"], light["e"], dif[:, 0:3], k, palette, c[:, 0:3])
                got = M.run_cpu_program(program[0], program[1], rec, depth, dims, origin, step, facing, bias, k, pts, nrm, colour, dif, c,
                                        palette, has_term)
                same = B.as_words(got) == B.as_words(want)
                assert same.all(), (name, n, facing, with_depth, bias, strength, np.argwhere(~same)[:4], got[~same.all(axis=1)][:2],
                                    want[~same.all(axis=1)][:2])
                off = (has_term == 0) | (light["probes"] <= 0)
                assert (B.as_words(want[off]) == B.as_words(colour[off])).all(), "a ray without a term keeps the colour's words"
                assert (B.as_words(want[:, 3]) == B.as_words(colour[:, 3])).all(), "alpha is the colour's"
                changed += (B.as_words(want) != B.as_words(colour)).any(axis=1).sum()
    assert changed > 100, "the fixture should light most rays"


def test_the_fixture_holds_what_it_promises():
    for name in MG.GRIDS:
        colour, dif, c, palette, has_term = M.ray_inputs(name, 257)
        assert set(palette) == {B.PLAIN, B.BULB, B.SPONGE} and has_term[0] and has_term[-1] and 0 < (has_term == 0).sum() < 64
        assert (B.as_words(colour) == 0x80000000).any() and (colour[:, 0:3] < 0).any() and (dif[:, 0:3] == 0).any()
        pts, nrm = MG.points(name, 257)
        light = G.grid_light(MG.records(name), *MG.GRIDS[name][0:3], pts, nrm, True)
        assert (light["probes"] == G.INVALID).any() and (light["e"][:, 0:3] < 0).any() and (light["e"][:, 0:3] > 0).any()


# ---------------------------------------------------------------- properties of the definition, through the program and the spec
def one_cell(e_value, hits=7):
    """A (2, 2, 2) grid whose eight probes hold sh[0] = e_value / K0 in every channel and zeros above: at a point with any normal
    e is about e_value in every channel (exactly a NaN for a NaN)."""
    rec = np.zeros(8, G.PROBE)
    rec["sh"][:, 0, :] = f32(e_value) / G.K0
    rec["hits"] = hits
    return rec, (2, 2, 2), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def run_one(program, rec, dims, origin, step, colour, dif, c, palette, strength=1.0):
    pts = np.array([[0.25, 0.5, 0.75, 0.0]], f32)
    nrm = np.array([[0.0, 0.0, 1.0, 0.0]], f32)
    k = B.scale_of(strength)
    light = G.grid_light(rec, dims, origin, step, pts, nrm, False)
    want = B.term(colour, [1], light["probes"], light["e"], dif[:, 0:3], k, [palette], c[:, 0:3])
    got = M.run_cpu_program(program[0], program[1], rec, None, dims, origin, step, False, 0.0, k, pts, nrm, colour, dif, c, [palette], [1])
    assert (B.as_words(got) == B.as_words(want)).all(), (got, want)
    return got, light


COLOUR = np.array([[0.25, -0.0, 1e-42, 2.0]], f32)
DIF = np.array([[0.5, 0.25, 1.0, 0.0]], f32)
PAL = np.array([[0.5, 0.125, 0.75, 0.0]], f32)


@pytest.mark.parametrize("e_value", [0.0, -0.0, -1.5, float("nan")])
def test_an_irradiance_that_is_not_positive_changes_no_number(program, e_value):
    """ec is +0, so ind is +0 in every channel: colour + 0 is colour as a number, and in every word but a −0's."""
    for palette in (B.PLAIN, B.BULB, B.SPONGE):
        got, light = run_one(program, *one_cell(e_value), COLOUR, DIF, PAL, palette)
        assert light["probes"][0] == 8
        if not np.isnan(e_value):
            assert (light["e"][0, 0:3] <= 0).all()
        assert (got == COLOUR).all() and B.as_words(got)[0, 0] == B.as_words(COLOUR)[0, 0] and B.as_words(got)[0, 2] == B.as_words(COLOUR)[0, 2]
        assert B.as_words(got)[0, 1] == 0, "−0 + +0 is +0: the one word an empty term may change"


def test_a_record_of_no_probe_changes_no_word(program):
    """Every corner invalid: probes = 0, and the colour's words stay — its −0 too, since no addition is performed."""
    for palette in (B.PLAIN, B.BULB, B.SPONGE):
        got, light = run_one(program, *one_cell(2.0, hits=G.INVALID), COLOUR, DIF, PAL, palette)
        assert light["probes"][0] == 0
        assert (B.as_words(got) == B.as_words(COLOUR)).all()


def test_the_palette_forms(program):
    """Plain x, bulb c·(x·8), sponge c·x, with x = (dif·e)·k, by hand on one point."""
    rec, dims, origin, step = one_cell(2.0)
    k = B.scale_of(0.5)
    out = {}
    for palette in (B.PLAIN, B.BULB, B.SPONGE):
        got, light = run_one(program, rec, dims, origin, step, COLOUR, DIF, PAL, palette, strength=0.5)
        out[palette] = got[0, 0:3]
        assert got[0, 3] == COLOUR[0, 3]
    e = light["e"][0, 0:3]
    assert (e > 0).all() and abs(float(e[0]) - 2.0) < 1e-5
    x = (DIF[0, 0:3] * e) * k
    assert x.dtype == f32
    assert (out[B.PLAIN] == COLOUR[0, 0:3] + x).all()
    assert (out[B.BULB] == COLOUR[0, 0:3] + PAL[0, 0:3] * (x * f32(8))).all()
    assert (out[B.SPONGE] == COLOUR[0, 0:3] + PAL[0, 0:3] * x).all()
    assert len({tuple(v) for v in out.values()}) == 3


def test_k_is_one_multiplication_by_the_headers_constant():
    assert B.INV_PI == f32(1 / np.pi) and B.scale_of(1.0) == B.INV_PI and B.scale_of(0.37) == f32(0.37) * B.INV_PI
    import abi_helpers as ah
    import re
    assert re.search(r"#define\s+RM_INV_PI\s+\(\(float\)0\.31830988618379067\)", ah.HEADER)
