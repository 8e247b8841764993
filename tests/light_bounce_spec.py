"""The term of rm_shade_rays_indirect (include/raymarcher_amd.h) in NumPy float32, written from the header's text and sharing no code
with the library: the clamp of the grid's irradiance, the products with the hit's diffuse colour and k = strength · RM_INV_PI, the
palette of the two fractals and the one addition to the shaded colour.  e comes from light_grid_spec / light_depth_spec (grid_e).
Every array below is float32 and every operation on them one rounded binary32 operation."""
import numpy as np

import light_depth_spec as D
import light_grid_spec as G

f32 = np.float32
INV_PI = f32(0.31830988618379067)  # RM_INV_PI: 1/π in binary64, rounded once
PLAIN, BULB, SPONGE = 0, 1, 2      # how the palette multiplies the term
assert INV_PI == f32(1.0 / np.pi)


def scale_of(strength):
    """k = strength · RM_INV_PI, one binary32 multiplication."""
    k = f32(strength) * INV_PI
    assert k.dtype == f32
    return k


def clamp_e(e):
    """ec = e > 0 ? e : +0 — negative values, −0 and NaN become +0."""
    e = np.asarray(e, f32)
    with np.errstate(invalid="ignore"):
        return np.where(e > f32(0), e, f32(0)).astype(f32)


def grid_e(probes, depth, dims, origin, step, points, normals, facing, normal_bias):
    """The grid record at (points, normals): rm_light_grid_irradiance_visible's where `depth` is given, rm_light_grid_irradiance's
    where it is None → GRIDLIGHT (m)."""
    if depth is None:
        return G.grid_light(probes, dims, origin, step, points, normals, facing)
    return D.grid_light_visible(probes, depth, dims, origin, step, points, normals, facing, normal_bias)


def indirect(dif, e, k, palette, c):
    """ind (m, 3): x = (dif · ec) · k, then c · (x · 8) on the Mandelbulb, c · x on the sponge, x elsewhere.  dif, e[:, 0:3], c:
    (m, 3) float32; palette: (m) of PLAIN / BULB / SPONGE; c is not read where the palette is PLAIN."""
    dif, c, k = np.asarray(dif, f32), np.asarray(c, f32), f32(k)
    ec = clamp_e(np.asarray(e, f32)[:, 0:3])
    palette = np.asarray(palette).reshape(-1, 1)
    with np.errstate(all="ignore"):
        x = (dif * ec) * k
        bulb = c * (x * f32(8))
        sponge = c * x
    assert x.dtype == f32 and bulb.dtype == f32 and sponge.dtype == f32
    return np.where(palette == BULB, bulb, np.where(palette == SPONGE, sponge, x)).astype(f32)


def term(colour, has_term, probes, e, dif, k, palette, c):
    """out (m, 4): colour.rgb + ind where the ray has a term — has_term (m): a valid ray whose primary march hit an object that is
    not emissive — and the grid record has probes > 0; colour's words, untouched, elsewhere.  Alpha is colour's."""
    colour = np.asarray(colour, f32)
    on = np.asarray(has_term, bool) & (np.asarray(probes) > 0)
    out = colour.copy()
    ind = indirect(dif, e, k, palette, c)
    with np.errstate(all="ignore"):
        lit = colour[:, 0:3] + ind
    assert lit.dtype == f32
    out[on, 0:3] = lit[on]
    return out


def as_words(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)
