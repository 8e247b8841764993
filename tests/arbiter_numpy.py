"""An INDEPENDENT arbiter for the headline pixel: the whole C3 fragment — vertex varyings, setScene, raymarch, sdScene with one
Mandelbulb, getNormal, pnoise / bumpNormal, softshadow, getPhong with directional lights, the orbit-trap colouring of render and
main's composite — written again from the SHADER TEXT (resources/raymarch.vert, resources/raymarch.frag of the reference;
`frag:N` below) in vectorised NumPy float64.

Why it exists (missing #2): the binary64 arbiter of oracle/rm_oracle_f64.c is the oracle's own C source compiled with
`#define float double` — a formula transcribed wrongly into rm_oracle.c would be wrong in both and pass.  This file shares no
source with the oracle: its own control flow (whole frames of rays advance together, finished rays drop out of the index set),
NumPy's arccos / arctan2 / sin / cos / power / log / sqrt, no rm_math contract.  It is test infrastructure only.

One sub-expression is evaluated in binary32 ON PURPOSE, as in the C arbiter: the hash → lattice-gradient map
of the classic Perlin noise (frag:1626-1644).  Its selector gz = 0.5 − |gx| − |gy| is an EXACT tie in real arithmetic for 7 of
the 49 hash classes, so which of two unrelated gradients `step(gz, 0)` picks is DEFINED by binary32 rounding in the shader (every
binary32 implementation with IEEE division agrees; a binary64 evaluation of that line picks other gradients for no meaningful
reason).  Those lines run on np.float32 arrays with NumPy's IEEE operations; everything around them is float64.

Scope: exactly what a frame of scenefiles/simple/unit_mandelbulb.json (C3) or unit_mengersponge.json (C5: sdMengerSponge,
frag:1049-1071, its palette and main's reflection loop, frag:2491-2524) executes with the reference's default #defines
(WHITE_BACKGROUND, PERLIN_BUMP; soft shadows, AO, refraction, sky box off): one object, DIRECTIONAL lights — render_frame — and,
at the end of the file, tables of any of sdMatch's nine primitives (untextured) under directional, point and spot lights with soft
shadows and ambient occlusion and main's reflection loop (C2's class: the geometry of 38 of the reference's scenefiles) —
render_frame_table — which also carries everything that reads RmResources, written from the shader text and the GL 3.3
specification: GL_LINEAR sampling of RGBA8 images with REPEAT and CLAMP_TO_EDGE (sample_rgba8), the four uv maps and getDiffuse's
blend (frag:1299-1398, 1746-1781), the sky box on the miss path (sample_cube, frag:2327), LTC area lights (IntegrateEdgeVec,
LTC_Evaluate, getAreaLight, the sample point and its shadow ray: frag:349-436, 1794-1822, 1884-1905), emissive rectangles (isAL,
UB5), the white / dark / no background and BrightColor (setBrightness).  The LTC tables are data: the 8-bit texels the reference
uploads.  No sub-expression of these paths needs binary32; one decision is DEFINED by it — the sphere's pole rule `v == 0 || v == 1`
(see uv_map).  With diag=True every pixel comes with margins: how far it lies from a place where the result jumps.  The sea, the
night sky, terrain, clouds and sdCUSTOM's tri-planar textures are not transcribed.  Anything else raises."""
import numpy as np

SURFACE_DIST = 1e-3          # frag:32
FRACTALS_BAILOUT = 2.0       # frag:30
BUMP_SCALE, BUMP_INTENSITY = 10.0, 2.0  # frag:128-129
RM_MANDELBULB, RM_MENGERSPONGE, RM_LIGHT_DIRECTIONAL = 10, 11, 1  # scenedata.h:18-33 / 10-15 ≡ frag:53-75
RM_FEAT_PERLIN_BUMP, RM_FEAT_WHITE_BACKGROUND = 128, 8  # include/raymarcher_amd.h: the shader's #defines as feature bits


def _dot(a, b):
    return (a * b).sum(-1)


def _normalize(v):
    return v / np.sqrt(_dot(v, v))[..., None]


def _mix(a, b, t):
    return a * (1.0 - t) + b * t


# ---------------------------------------------------------------------------------------------- frag:775-803
def sd_mandelbulb(pos, power, iters, julia=(0.0, 0.0)):
    """sdMandelBulb: returns (distance estimate, resColor = (m, trap.y, trap.z, trap.w)).  A point that has bailed out stops
    updating (the shader's `break`)."""
    w = np.array(pos, dtype=np.float64)
    c = w.copy()
    if np.hypot(*julia) != 0.0:  # frag:782-784
        c = np.broadcast_to(np.array([julia[0], julia[1], 0.0]), w.shape).copy()
    m = _dot(w, w)
    trap = np.concatenate([np.abs(w), m[:, None]], -1)
    dz = np.ones(len(w))
    live = np.ones(len(w), dtype=bool)
    with np.errstate(all="ignore"):
        for _ in range(iters):
            dz_n = power * np.power(m, (power - 1.0) / 2.0) * dz + 1.0
            r = np.sqrt(_dot(w, w))
            b = power * np.arccos(w[:, 1] / r)
            a = power * np.arctan2(w[:, 0], w[:, 2])
            w_n = c + np.power(r, power)[:, None] * np.stack([np.sin(b) * np.sin(a), np.cos(b), np.sin(b) * np.cos(a)], -1)
            trap_n = np.minimum(trap, np.concatenate([np.abs(w_n), m[:, None]], -1))
            m_n = _dot(w_n, w_n)
            dz = np.where(live, dz_n, dz)
            w = np.where(live[:, None], w_n, w)
            trap = np.where(live[:, None], trap_n, trap)
            m = np.where(live, m_n, m)
            live = live & ~(m > FRACTALS_BAILOUT)
            if not live.any():
                break
        d = 0.25 * np.log(m) * np.sqrt(m) / dz
    return d, np.concatenate([m[:, None], trap[:, 1:]], -1)


# ---------------------------------------------------------------------------------------------- frag:1586-1676
def _permute(x):  # frag:1602-1604; exact integers below 2^24 in either precision
    return np.mod((x * 34.0 + 1.0) * x, 289.0)


def _lattice_gradients32(ixy):
    """frag:1626-1634 (and 1636-1644) on np.float32 arrays: the hash → gradient map whose tie-break binary32 defines."""
    f = np.float32
    ixy = ixy.astype(f)
    gx = ixy / f(7.0)
    t = np.floor(gx) / f(7.0)
    gy = (t - np.floor(t)) - f(0.5)
    gx = gx - np.floor(gx)
    gz = f(0.5) - np.abs(gx) - np.abs(gy)
    sz = (gz <= f(0.0)).astype(f)                       # step(gz, 0)
    gx = gx - sz * ((gx >= f(0.0)).astype(f) - f(0.5))  # step(0, gx)
    gy = gy - sz * ((gy >= f(0.0)).astype(f) - f(0.5))
    return gx.astype(np.float64), gy.astype(np.float64), gz.astype(np.float64)


def pnoise(p):
    """Classic Perlin noise, 3-D (frag:1610-1676)."""
    p = np.asarray(p, dtype=np.float64)
    Pi0 = np.floor(p)
    Pi1 = np.mod(Pi0 + 1.0, 256.0)
    Pi0 = np.mod(Pi0, 256.0)
    Pf0 = p - np.floor(p)
    Pf1 = Pf0 - 1.0
    n = {}
    for cz in (0, 1):
        iz = (Pi1 if cz else Pi0)[:, 2]
        for cy in (0, 1):
            iy = (Pi1 if cy else Pi0)[:, 1]
            for cx in (0, 1):
                ix = (Pi1 if cx else Pi0)[:, 0]
                gx, gy, gz = _lattice_gradients32(_permute(_permute(_permute(ix) + iy) + iz))
                g = np.stack([gx, gy, gz], -1)
                g = g * (1.79284291400159 - 0.85373472095314 * _dot(g, g))[:, None]  # taylorInvSqrt, frag:1606-1608
                off = np.stack([(Pf1 if cx else Pf0)[:, 0], (Pf1 if cy else Pf0)[:, 1], (Pf1 if cz else Pf0)[:, 2]], -1)
                n[(cx, cy, cz)] = _dot(g, off)
    t = Pf0
    fade = t * t * t * (t * (t * 6.0 - 15.0) + 10.0)  # frag:1587-1589
    nz = {(cx, cy): _mix(n[(cx, cy, 0)], n[(cx, cy, 1)], fade[:, 2]) for cx in (0, 1) for cy in (0, 1)}
    ny = {cx: _mix(nz[(cx, 0)], nz[(cx, 1)], fade[:, 1]) for cx in (0, 1)}
    return 2.2 * _mix(ny[0], ny[1], fade[:, 0])


def bump_normal(normal, pos, scale=BUMP_SCALE, intensity=BUMP_INTENSITY):  # frag:1679-1691
    q = pos * scale
    n0 = pnoise(q)
    grad = np.stack([pnoise(q + np.array([0.1, 0.0, 0.0])) - n0, pnoise(q + np.array([0.0, 0.1, 0.0])) - n0,
                     pnoise(q + np.array([0.0, 0.0, 0.1])) - n0], -1)
    return _normalize(normal + grad * intensity)


# ---------------------------------------------------------------------------------------------- the frame
class Bulb:
    """What sdScene (frag:1406-1430) does with a table of one Mandelbulb: object-space point, estimate × scaleFactor."""

    def __init__(self, inv_model, scale_factor, power, iters, julia):
        self.M, self.sf, self.power, self.iters, self.julia = np.asarray(inv_model, np.float64), float(scale_factor), float(power), int(iters), julia

    def __call__(self, p):
        po = p @ self.M[:3, :3].T + self.M[:3, 3]  # vec3(invModelMatrix · vec4(p, 1)), frag:1417
        d, res = sd_mandelbulb(po, self.power, self.iters, self.julia)
        return d * self.sf, res


def raymarch(sd, ro, rd, end, max_steps, shadow=False):
    """frag:1453-1484 (shadow=False, side = +1) and the march of frag:1703-1725 (shadow=True: t += |d|, start at mint = 0).
    Returns (hit, depth as raymarch reports it: rayDepth − minD, trap of the last evaluation)."""
    n = len(ro)
    t = np.zeros(n)
    d = np.full(n, 1000000.0)
    trap = np.zeros((n, 4))
    idx = np.arange(n)
    for _ in range(max_steps):
        if len(idx) == 0:
            break
        dd, tr = sd(ro[idx] + rd[idx] * t[idx, None])
        d[idx], trap[idx] = dd, tr
        stop = (np.abs(dd) < SURFACE_DIST) | (t[idx] > end)
        go = ~stop
        t[idx[go]] += np.abs(dd[go]) if shadow else dd[go]
        idx = idx[go]
    hit = np.abs(d) < SURFACE_DIST
    return hit, t - d, trap


def get_normal(sd, p):  # frag:1436-1444
    e = np.array([1.0, -1.0, 0.0]) * 0.5773 * 0.0005
    x, y = e[0], e[1]
    taps = [np.array([x, y, y]), np.array([y, y, x]), np.array([y, x, y]), np.array([x, x, x])]  # e.xyy, e.yyx, e.yxy, e.xxx
    acc = np.zeros_like(p)
    for k in taps:
        acc = acc + k * sd(p + k)[0][:, None]
    return _normalize(acc)


def get_phong(sd, N, obj, lights, g, p, rd, far, max_steps):
    """frag:1842-1933 for an untextured object and DIRECTIONAL lights, soft shadows and ambient occlusion off."""
    ka, kd, ks = g
    total = np.broadcast_to(obj["cAmbient"] * ka, p.shape).copy()  # ao = 1
    V = _normalize(-rd)
    for li in lights:
        L = np.broadcast_to(_normalize(-li["dir"]), p.shape)
        occluded, _, _ = raymarch(sd, p + N * SURFACE_DIST * 5.0, L, far, max_steps, shadow=True)  # frag:1908
        ndl = _dot(N, L)
        lit = ~occluded & ~(ndl <= 0.005)  # frag:1909-1912
        col = (kd * obj["cDiffuse"]) * np.clip(ndl, 0.0, 1.0)[:, None] * li["color"]  # getDiffuse, texLoc == −1: frag:1749-1752
        R = (-L) - 2.0 * _dot(N, -L)[:, None] * N  # reflect(−L, N)
        rdv = np.clip(_dot(R, V), 0.0, 1.0)
        spec = ks * rdv if obj["shininess"] == 0 else ks * np.power(rdv, obj["shininess"])  # frag:1787-1792
        col = col + spec[:, None] * obj["cSpecular"] * li["color"]
        total = total + np.where(lit[:, None], col, 0.0)  # fAtt = aFall = 1 for a directional light
    return total


class Menger:
    """sdScene with a table of one Menger sponge (frag:1406-1430, 1049-1071).  `levels` is the loop bound of frag:1056 (4 in the
    shader, a build knob of the product); resColor = (d, min(0.2·da·db·dc), (1 + m)/4, 0) of the last level that raised d."""

    def __init__(self, inv_model, scale_factor, levels, itime):
        self.M, self.sf, self.levels, self.itime = np.asarray(inv_model, np.float64), float(scale_factor), int(levels), float(itime)

    def __call__(self, p):
        p = p @ self.M[:3, :3].T + self.M[:3, 3]
        q = np.abs(p) - 1.0                                        # sdBox(p, vec3(1)), frag:843-846
        d = np.sqrt(_dot(np.maximum(q, 0.0), np.maximum(q, 0.0))) + np.minimum(np.max(q, axis=-1), 0.0)
        res = np.stack([d, np.ones_like(d), np.zeros_like(d), np.zeros_like(d)], -1)
        x = -np.cos(0.5 * self.itime)                              # smoothstep(−0.2, 0.2, −cos(0.5·iTime)), frag:1052
        t = np.clip((x + 0.2) / 0.4, 0.0, 1.0)
        ani = t * t * (3.0 - 2.0 * t)
        off = 1.5 * np.sin(0.01 * self.itime)
        ma = np.array([[0.60, 0.00, -0.80], [0.00, 1.00, 0.00], [0.80, 0.00, 0.60]])  # columns (.6,0,.8), (0,1,0), (−.8,0,.6): frag:124-126
        s = 1.0
        for m in range(self.levels):
            p = _mix(p, (p + off) @ ma.T, ani)                     # frag:1057
            a = np.mod(p * s, 2.0) - 1.0
            s *= 3.0
            r = np.abs(1.0 - 3.0 * np.abs(a))
            da, db, dc = np.maximum(r[:, 0], r[:, 1]), np.maximum(r[:, 1], r[:, 2]), np.maximum(r[:, 2], r[:, 0])
            c = (np.minimum(da, np.minimum(db, dc)) - 1.0) / s
            up = c > d
            d = np.where(up, c, d)
            res = np.where(up[:, None], np.stack([d, np.minimum(res[:, 1], 0.2 * da * db * dc), np.full_like(d, (1.0 + m) / 4.0),
                                                   np.zeros_like(d)], -1), res)
        return d * self.sf, res


def render_rays(sd, kind, obj, lights, g, ro, rd, far, settings, bg):
    """render() (frag:2318-2375) for a batch of rays: (rgb, isEnv, hit point, shading normal).  Point and normal are only
    meaningful where isEnv is False (the `out IntersectionInfo` of a hit)."""
    n = len(ro)
    rgb = np.broadcast_to(bg, (n, 3)).copy()                # a miss: vec4(bgCol, 1), frag:2323-2329
    hit, depth, trap = raymarch(sd, ro, rd, far, settings.maxSteps)
    P, N = np.zeros((n, 3)), np.zeros((n, 3))
    if hit.any():
        p = ro[hit] + rd[hit] * depth[hit, None]             # frag:2333
        pn = get_normal(sd, p)
        if settings.features & RM_FEAT_PERLIN_BUMP:          # #define PERLIN_BUMP (frag:15, 2334-2336)
            pn = bump_normal(pn, p)
        ph = get_phong(sd, pn, obj, lights, (g.ka, g.kd, g.ks), p, rd[hit], far, settings.maxSteps)
        tr = trap[hit]
        if kind == "bulb":                                   # frag:2354-2361
            col = np.full((len(p), 3), 0.2)
            col = _mix(col, np.array([0.10, 0.20, 0.30]), np.clip(tr[:, 1], 0.0, 1.0)[:, None])
            col = _mix(col, np.array([0.02, 0.10, 0.30]), np.clip(tr[:, 2] * tr[:, 2], 0.0, 1.0)[:, None])
            col = _mix(col, np.array([0.30, 0.10, 0.02]), np.clip(np.power(tr[:, 3], 6.0), 0.0, 1.0)[:, None])
            col = col * 0.5
            col = col * (ph * 8.0)
        else:                                                # MENGERSPONGE, frag:2362-2365
            col = (0.5 + 0.5 * np.cos(np.array([0.0, 1.0, 2.0]) + 2.0 * tr[:, 2:3])) * ph
        rgb[hit], P[hit], N[hit] = col, p, pn
    return rgb, ~hit, P, N


def render_frame(tables, settings, W, H):
    """fragColor of every pixel, (H, W, 4) float64, row 0 = bottom (gl_FragCoord convention): a table of one Mandelbulb or one
    Menger sponge under directional lights; main's reflection loop (frag:2491-2524) when it is enabled."""
    assert tables.num_objects == 1 and tables.objects[0].type in (RM_MANDELBULB, RM_MENGERSPONGE) and tables.objects[0].texLoc == -1
    assert not (settings.enableSoftShadow or settings.enableAmbientOcclusion or settings.enableRefraction or settings.enableSkyBox)
    assert not tables.globals_.isTwoD and settings.features & RM_FEAT_WHITE_BACKGROUND
    o = tables.objects[0]
    obj = {"cAmbient": np.array(list(o.cAmbient), np.float64), "cDiffuse": np.array(list(o.cDiffuse), np.float64),
           "cSpecular": np.array(list(o.cSpecular), np.float64), "shininess": float(o.shininess)}
    c_refl = np.array(list(o.cReflective), np.float64)
    assert not o.isEmissive
    lights = []
    for i in range(tables.num_lights):
        li = tables.lights[i]
        assert li.type == RM_LIGHT_DIRECTIONAL
        lights.append({"dir": np.array(list(li.dir), np.float64), "color": np.array(list(li.color), np.float64)})
    gl = tables.globals_
    inv_model = np.array(list(o.invModel), np.float64).reshape(4, 4).T
    if o.type == RM_MANDELBULB:
        kind, sd = "bulb", Bulb(inv_model, o.scaleFactor, gl.power, settings.fractalIters, (gl.juliaSeed[0], gl.juliaSeed[1]))
    else:
        kind, sd = "menger", Menger(inv_model, o.scaleFactor, settings.mengerLevels, gl.iTime)
    inv_pv = np.array(list(tables.camera.invProjView), np.float64).reshape(4, 4).T  # column-major storage
    far = float(tables.camera.initialFar)
    # raymarch.vert:13-25: nearClip / farClip are affine in the quad position, so their interpolated value at a pixel centre
    # IS the matrix product at that position (in real arithmetic; DESIGN.md §2.3 is about binary32)
    ys, xs = np.mgrid[0:H, 0:W]
    ndc = np.stack([(xs.ravel() + 0.5) / W * 2.0 - 1.0, (ys.ravel() + 0.5) / H * 2.0 - 1.0], -1)
    near = np.concatenate([ndc, np.full((len(ndc), 1), -1.0), np.ones((len(ndc), 1))], -1) @ inv_pv.T
    farc = np.concatenate([ndc, np.ones((len(ndc), 1)), np.ones((len(ndc), 1))], -1) @ inv_pv.T
    ro = near[:, :3] / near[:, 3:]                      # setScene, frag:2388-2392
    rd = _normalize(farc[:, :3] / farc[:, 3:] - ro)
    bg = np.array([1.0, 1.0, 1.0])                      # WHITE_BACKGROUND, frag:2414-2416
    out = np.ones((len(ndc), 4))
    rgb, is_env, P, N = render_rays(sd, kind, obj, lights, gl, ro, rd, far, settings, bg)  # frag:2443
    out[:, :3] = rgb                                    # a miss returns here (frag:2459-2465); a hit: phong = ri.fragColor
    if settings.enableReflection and np.sqrt(_dot(c_refl, c_refl)) != 0.0:  # frag:2491-2524
        idx = np.nonzero(~is_env)[0]
        p, n, d = P[idx], N[idx], rd[idx]
        fil = np.ones(3)
        for _ in range(settings.numReflection):
            if len(idx) == 0:
                break
            r = d - 2.0 * _dot(n, d)[:, None] * n       # reflect(info.rd, info.n)
            sro = p + r * SURFACE_DIST * 3.0
            fil = fil * c_refl                          # the FIRST hit's material throughout (frag:2500-2501), one object here
            rgb, env, P2, N2 = render_rays(sd, kind, obj, lights, gl, sro, r, far, settings, bg)
            out[idx, :3] += gl.ks * fil * rgb           # refl += vec4(ks·fil·res.rgb, 1)
            out[idx, 3] += 1.0
            go = ~env                                   # `if (res.isEnv) break;`
            idx, p, n, d = idx[go], P2[go], N2[go], r[go]
    return out.reshape(H, W, 4), (~is_env).reshape(H, W)


# ---------------------------------------------------------------------------------------------- tables of primitives (C2)
# Round 4, late: the lighting configuration (scenefiles/lighting/directional_light_2.json with soft shadows and ambient occlusion)
# transcribed independently as well — sdScene over a table (frag:1406-1430), sdMatch's nine primitives (frag:832-896, 991-1019,
# 1262-1280), softshadow with its penumbra factor (frag:1703-1725; UB1 of DESIGN.md §4: r.d is the factor on a miss too), calcAO
# (frag:1729-1740), getPhong with directional, point and spot lights (frag:1842-1933, 439-461).
RM_CUBE, RM_CONE, RM_CYLINDER, RM_SPHERE, RM_LIGHT_POINT, RM_LIGHT_SPOT = 0, 1, 2, 3, 0, 2
RM_FEAT_SKY_BACKGROUND, RM_FEAT_NIGHTSKY_BACKGROUND, RM_FEAT_DARK_BACKGROUND = 1, 2, 4
RM_FEAT_CLOUD, RM_FEAT_TERRAIN, RM_FEAT_SEA = 16, 32, 64


def _len2(a, b):
    return np.sqrt(a * a + b * b)


def sd_cube(p):      # sdBox(p, vec3(0.5)), frag:843-846
    q = np.abs(p) - 0.5
    return np.sqrt(_dot(np.maximum(q, 0.0), np.maximum(q, 0.0))) + np.minimum(np.max(q, axis=-1), 0.0)


def sd_cone(p, r=0.5, h=0.5):  # frag:853-862
    po = np.stack([_len2(p[:, 0], p[:, 2]) - r, p[:, 1] + h], -1)
    e = np.array([-r, 2.0 * h])
    q = po - e * np.clip((po @ e) / (e @ e), 0.0, 1.0)[:, None]
    d = _len2(q[:, 0], q[:, 1])
    return np.where(np.maximum(q[:, 0], q[:, 1]) > 0.0, d, -np.minimum(d, po[:, 1]))


def sd_cylinder(p, h=0.5, r=0.5):  # frag:869-872
    d = np.abs(np.stack([_len2(p[:, 0], p[:, 2]), p[:, 1]], -1)) - np.array([r, h])
    return np.minimum(np.maximum(d[:, 0], d[:, 1]), 0.0) + _len2(np.maximum(d[:, 0], 0.0), np.maximum(d[:, 1], 0.0))


def sd_sphere(p, r=0.5):  # frag:832-834
    return np.sqrt(_dot(p, p)) - r


def sd_octahedron(p, s=0.5):  # frag:877-888
    p = np.abs(p)
    m = p[:, 0] + p[:, 1] + p[:, 2] - s
    r = 3.0 * p - m[:, None]
    q = np.where((r[:, 0] < 0.0)[:, None], p, np.where((r[:, 1] < 0.0)[:, None], p[:, [1, 2, 0]], p[:, [2, 0, 1]]))
    k = np.clip(0.5 * (q[:, 2] - q[:, 1] + s), 0.0, s)
    inside = np.sqrt(q[:, 0] ** 2 + (q[:, 1] - s + k) ** 2 + (q[:, 2] - k) ** 2)
    return np.where((r[:, 0] < 0.0) | (r[:, 1] < 0.0) | (r[:, 2] < 0.0), inside, m * 0.57735027)


def sd_torus(p, t=(0.5, 0.5 / 4)):  # frag:893-896
    return _len2(_len2(p[:, 0], p[:, 2]) - t[0], p[:, 1]) - t[1]


def sd_capsule(p, h=0.5, r=0.1):  # frag:991-994
    y = p[:, 1] - np.clip(p[:, 1], 0.0, h)
    return np.sqrt(p[:, 0] ** 2 + y ** 2 + p[:, 2] ** 2) - r


def sd_deathstar(p2, ra=0.5, rb=0.35, d=0.5):  # frag:1005-1019
    px, py = p2[:, 0], _len2(p2[:, 1], p2[:, 2])
    a = (ra * ra - rb * rb + d * d) / (2.0 * d)
    b = np.sqrt(max(ra * ra - a * a, 0.0))
    rim = _len2(px - a, py - b)
    body = np.maximum(_len2(px, py) - ra, -(_len2(px - d, py) - rb))
    return np.where(px * b - py * a > d * np.maximum(b - py, 0.0), rim, body)


def sd_rectangle(p):  # sdBox(p, vec3(0.5, 0.5, 0)), frag:1279
    q = np.abs(p) - np.array([0.5, 0.5, 0.0])
    return np.sqrt(_dot(np.maximum(q, 0.0), np.maximum(q, 0.0))) + np.minimum(np.max(q, axis=-1), 0.0)


def sd_sierpinski(p):  # frag:807-826: 14 fold-and-scale iterations (Scale 1.85, Offset 2), length(p)·Scale^−14
    # Scale is the shader's binary32 constant 1.85 (1.850000023841858): fourteen scalings amplify the 2.4e-8 between it and the
    # binary64 1.85 to 1e-3 of a pixel — the constant is part of the function, not of the precision it is evaluated in
    scale = float(np.float32(1.85))
    p = p.copy()
    for _ in range(14):
        f = p[:, 0] + p[:, 1] < 0.0
        p[f, 0], p[f, 1] = -p[f, 1], -p[f, 0]       # p.xy = −p.yx
        f = p[:, 0] + p[:, 2] < 0.0
        p[f, 0], p[f, 2] = -p[f, 2], -p[f, 0]       # p.xz = −p.zx
        f = p[:, 1] + p[:, 2] < 0.0
        p[f, 2], p[f, 1] = -p[f, 1], -p[f, 2]       # p.zy = −p.yz
        p = p * scale - 2.0 * (scale - 1.0)
    return np.sqrt(_dot(p, p)) * np.power(scale, -14.0)


class Table:
    """sdScene (frag:1406-1430) over a table of primitives: the minimum of sdMatch(po)·scaleFactor with a strict `<` (the first of
    equal objects wins); the index of the minimum travels in the first component of what the fractal classes call the trap."""
    SDF = {RM_CUBE: sd_cube, RM_CONE: sd_cone, RM_CYLINDER: sd_cylinder, RM_SPHERE: sd_sphere, 4: sd_octahedron, 5: sd_torus,
           6: sd_capsule, 7: sd_deathstar, 8: sd_rectangle, 12: sd_sierpinski}  # scenedata.h's PrimitiveType order ≡ frag:53-66

    def __init__(self, objects):
        self.objs = [(self.SDF[t], np.asarray(M, np.float64), float(sf)) for t, M, sf in objects]

    def __call__(self, p):
        best = np.full(len(p), 1000000.0)
        idx = np.full(len(p), -1.0)
        for k, (f, M, sf) in enumerate(self.objs):
            d = f(p @ M[:3, :3].T + M[:3, 3]) * sf
            closer = d < best
            best, idx = np.where(closer, d, best), np.where(closer, float(k), idx)
        return best, np.stack([idx, np.zeros_like(idx), np.zeros_like(idx), np.zeros_like(idx)], -1)


def softshadow(sd, ro, rd, maxt, max_steps, k=8.0):
    """frag:1703-1725 with mint = 0: (hit, res, intersectObj, margin).  res = min over the steps of k·d/t — the first step divides
    by t = 0: +inf for d > 0, which min drops, as in the shader.  intersectObj is the closest object of the last evaluation (−1 on a
    miss); margin = min over the evaluations of | |d| − SURFACE_DIST | (world units): how near the march came to the hit test's jump."""
    n = len(ro)
    t, res, d = np.zeros(n), np.ones(n), np.full(n, 1000000.0)
    obj, margin = np.full(n, -1), np.full(n, np.inf)
    idx = np.arange(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        for _ in range(max_steps):
            if len(idx) == 0:
                break
            dd, tr = sd(ro[idx] + rd[idx] * t[idx, None])
            d[idx], obj[idx] = dd, tr[:, 0].astype(int)
            margin[idx] = np.minimum(margin[idx], np.abs(np.abs(dd) - SURFACE_DIST))
            go = ~((np.abs(dd) < SURFACE_DIST) | (t[idx] > maxt[idx]))
            g = idx[go]
            res[g] = np.minimum(res[g], k * dd[go] / t[g])
            t[g] += np.abs(dd[go])
            idx = g
    hit = np.abs(d) < SURFACE_DIST
    return hit, res, np.where(hit, obj, -1), margin


def calc_ao(sd, pos, nor):  # frag:1729-1740
    occ, sca = np.zeros(len(pos)), 1.0
    live = np.ones(len(pos), bool)
    for i in range(5):
        hgt = 0.01 + 0.12 * float(i) / 4.0
        d = sd(pos + hgt * nor)[0]
        occ = np.where(live, occ + (hgt - d) * sca, occ)
        sca *= 0.95
        live = live & ~(occ > 0.35)
    return np.clip(1.0 - 3.0 * occ, 0.0, 1.0) * (0.5 + 0.5 * nor[:, 1])


def get_phong_table(sd, N, mats, lights, g, p, rd, far, settings, k=None, dif=None, ltc=None, margins=None):
    """frag:1842-1933: (one material ROW per point in `mats`) directional, point and spot lights with the soft shadow factor and
    ambient occlusion when the settings ask for them, and AREA lights (frag:1884-1905) through getAreaLight with `ltc` = (LTC1, LTC2).
    `dif` is getDiffuse at every point (kd·cDiffuse for untextured objects); `k` the object of every point (the `lightIdx != i` test
    of an area light's shadow ray reads the object table `mats`).  `margins` (dict of per-point arrays, updated in place): "geom" the
    shadow marches' hit-test margins, "cos" |N·L − 0.005| (the `NdotL <= 0.005` jump) and the LTC `behind` test's |cos|."""
    ka, kd, ks = g
    if dif is None:
        dif = kd * mats["cDiffuse"]
    ao = calc_ao(sd, p, N) if settings.enableAmbientOcclusion else np.ones(len(p))
    total = mats["cAmbient"] * ka * ao[:, None]
    V = _normalize(-rd)
    for i, li in enumerate(lights):
        if li["type"] == RM_LIGHT_AREA:
            pts = li["points"]
            rp = pts[0] + rd[:, 0:1] * (pts[1] - pts[0]) + rd[:, 1:2] * (pts[3] - pts[0])  # vec2(rd + idx), idx = 0, frag:425-436
            to = rp - p
            L = _normalize(to)
            ndl = _dot(N, L)
            occluded, _pen, hit_obj, sm = softshadow(sd, p + N * SURFACE_DIST * 5.0, L, np.sqrt(_dot(to, to)), settings.maxSteps)
            other = occluded & (mats["lightIdx_table"][np.maximum(hit_obj, 0)] != i)
            lit = ~(ndl <= 0.005) & ~other
            col, cm = get_area_light(N, V, p, li, mats["cSpecular"], dif, ltc)
            total = total + np.where(lit[:, None], col, 0.0)
            if margins is not None:
                margins["geom"] = np.minimum(margins["geom"], np.where(ndl <= 0.005, np.inf, sm))
                margins["cos"] = np.minimum(margins["cos"], np.minimum(np.abs(ndl - 0.005), np.where(lit, cm, np.inf)))
            continue
        if li["type"] in (RM_LIGHT_POINT, RM_LIGHT_SPOT):
            to = li["pos"] - p
            dist = np.sqrt(_dot(to, to))
            L, maxt = to / dist[:, None], dist
            f = li["func"]
            with np.errstate(divide="ignore"):
                f_att = np.minimum(1.0 / (f[0] + dist * f[1] + dist * dist * f[2]), 1.0)  # attenuationFactor, frag:445-447
            if li["type"] == RM_LIGHT_SPOT:  # angularFalloff, frag:439-461
                cosalpha = _dot(np.broadcast_to(-_normalize(li["dir"]), p.shape), L)
                inner = li["angle"] - li["penumbra"]
                tt = (np.arccos(np.clip(cosalpha, -1.0, 1.0)) - inner) / (li["angle"] - inner)
                fall = 1.0 - (-2.0 * tt ** 3 + 3.0 * tt ** 2)
                f_att = f_att * np.where(cosalpha <= np.cos(li["angle"]), 0.0, np.where(cosalpha > np.cos(inner), 1.0, fall))
        else:
            L = np.broadcast_to(_normalize(-li["dir"]), p.shape)
            maxt, f_att = np.full(len(p), far), np.ones(len(p))
        occluded, pen, _o, sm = softshadow(sd, p + N * SURFACE_DIST * 5.0, L, maxt, settings.maxSteps)  # frag:1908
        ndl = _dot(N, L)
        lit = ~occluded & ~(ndl <= 0.005)
        col = dif * np.clip(ndl, 0.0, 1.0)[:, None] * li["color"]
        R = (-L) - 2.0 * _dot(N, -L)[:, None] * N
        rdv = np.clip(_dot(R, V), 0.0, 1.0)
        sh = mats["shininess"]
        with np.errstate(invalid="ignore"):
            spec = np.where(sh == 0.0, ks * rdv, ks * np.power(rdv, np.where(sh == 0.0, 1.0, sh)))  # getSpecular, frag:1787-1792
        col = (col + spec[:, None] * mats["cSpecular"] * li["color"]) * f_att[:, None]
        if settings.enableSoftShadow:
            col = col * pen[:, None]  # frag:1928 (UB1: the penumbra factor, hit or miss)
        total = total + np.where(lit[:, None], col, 0.0)
        if margins is not None:
            margins["geom"] = np.minimum(margins["geom"], sm)
            margins["cos"] = np.minimum(margins["cos"], np.where(occluded, np.inf, np.abs(ndl - 0.005)))
    return total

def _refract(I, Nn, eta):  # GLSL refract (spec 8.5): k = 1 − η²(1 − (N·I)²); k < 0 → 0, else η·I − (η·(N·I) + √k)·N
    eta = np.asarray(eta, np.float64) * np.ones(len(I))
    ni = _dot(Nn, I)
    k = 1.0 - eta * eta * (1.0 - ni * ni)
    with np.errstate(invalid="ignore"):
        r = eta[:, None] * I - (eta * ni + np.sqrt(k))[:, None] * Nn
    return np.where((k < 0.0)[:, None], 0.0, r)


def _raymarch_depth(sd, ro, rd, end, max_steps, side):
    """raymarch(…).d (frag:1453-1484) with `side`: rayDepth − minD on a hit, rayDepth on a miss (UB2)."""
    n = len(ro)
    t, d = np.zeros(n), np.full(n, 1000000.0)
    idx = np.arange(n)
    for _ in range(max_steps):
        if len(idx) == 0:
            break
        dd = sd(ro[idx] + rd[idx] * t[idx, None])[0]
        d[idx] = dd
        go = ~((np.abs(dd) < SURFACE_DIST) | (t[idx] > end))
        t[idx[go]] += dd[go] * side
        idx = idx[go]
    return np.where(np.abs(d) < SURFACE_DIST, t - d, t)


# ---------------------------------------------------------------------------------------------- samplers, uv maps, area lights
# Written from the shader text and the GL 3.3 specification (§3.8.10 cube-map face selection, §3.8.11 GL_LINEAR, table 3.22 wrap
# modes).  Images are uint8 (rows, columns, 4) arrays in upload order: row j holds t ∈ [j, j + 1)/rows (RmTexture).
RM_LIGHT_AREA = 3
TEXTURE_EPS = 0.005                       # frag:37
GL_PI = float(np.float32(3.14159265))     # frag:41: a binary32 constant of the shader — the value, not a precision choice
LUT_SIZE = 64.0                           # frag:47-49
LUT_SCALE, LUT_BIAS = (LUT_SIZE - 1.0) / LUT_SIZE, 0.5 / LUT_SIZE
BRIGHT_FILTER = np.array([0.2126, 0.7152, 0.0722])  # frag:78
REPEAT, CLAMP_TO_EDGE = "repeat", "clamp"


def sample_rgba8(img, s, t, wrap):
    """texture(sampler2D, (s, t)) of an RGBA8 image with GL_LINEAR filtering (GL 3.3 §3.8.11): u = s·W − ½, i0 = ⌊u⌋, α = u − i0
    (texel centres at i + ½), the four texels weighted (1−α)(1−β), α(1−β), (1−α)β, αβ, texel = byte / 255.  `wrap`: REPEAT takes
    every index mod W (negative ones too: −1 → W − 1), CLAMP_TO_EDGE clamps it to [0, W − 1].  Returns (n, 4) float64."""
    img = np.asarray(img)
    rows, cols = img.shape[:2]
    u = np.asarray(s, np.float64) * cols - 0.5
    v = np.asarray(t, np.float64) * rows - 0.5
    i0, j0 = np.floor(u), np.floor(v)
    a, b = (u - i0)[:, None], (v - j0)[:, None]

    def index(i, n):
        return (np.mod(i, n) if wrap == REPEAT else np.clip(i, 0, n - 1)).astype(np.int64)
    i0, i1, j0, j1 = index(i0, cols), index(i0 + 1, cols), index(j0, rows), index(j0 + 1, rows)
    tex = img.astype(np.float64) / 255.0
    return ((1 - a) * (1 - b) * tex[j0, i0] + a * (1 - b) * tex[j0, i1] + (1 - a) * b * tex[j1, i0] + a * b * tex[j1, i1])


def sample_cube(faces, r):
    """texture(samplerCube, r) (GL 3.3 §3.8.10, table 3.19) → (rgb, margin).  The major axis is the largest |component|; equal
    magnitudes resolve x before y before z (the spec leaves ties to the implementation).  Faces +X, −X, +Y, −Y, +Z, −Z:
    (sc, tc) = (−rz, −ry), (rz, −ry), (rx, rz), (rx, −rz), (rx, −ry), (−rx, −ry); s = (sc/|ma| + 1)/2, t = (tc/|ma| + 1)/2, filtered
    inside the face with CLAMP_TO_EDGE (seamless filtering is never enabled).  margin: texels between (s, t) and the face's nearest
    edge — where the face, and so the colour, jumps."""
    r = np.asarray(r, np.float64)
    ab = np.abs(r)
    ax_ = np.where((ab[:, 0] >= ab[:, 1]) & (ab[:, 0] >= ab[:, 2]), 0, np.where(ab[:, 1] >= ab[:, 2], 1, 2))
    ma = ab[np.arange(len(r)), ax_]
    pos = r[np.arange(len(r)), ax_] >= 0.0
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    sc = np.select([(ax_ == 0) & pos, ax_ == 0, ax_ == 1, (ax_ == 2) & pos], [-z, z, x, x], -x)
    tc = np.select([ax_ == 0, (ax_ == 1) & pos, ax_ == 1], [-y, z, -z], -y)
    face = 2 * ax_ + (~pos).astype(int)
    s, t = (sc / ma + 1.0) / 2.0, (tc / ma + 1.0) / 2.0
    rgb, margin = np.zeros((len(r), 3)), np.zeros(len(r))
    for f in range(6):
        sel = face == f
        if sel.any():
            n = faces[f].shape[0]
            rgb[sel] = sample_rgba8(faces[f], s[sel], t[sel], CLAMP_TO_EDGE)[:, :3]
            margin[sel] = np.minimum(np.minimum(s[sel], 1 - s[sel]), np.minimum(t[sel], 1 - t[sel])) * n
    return rgb, margin


def _u_from_theta(theta):
    """frag:1346-1350 (and 1369-1373, 1385-1389): u = −θ/2π for θ < 0, 1 − θ/2π otherwise.  It is continuous at θ = ±π (both give
    ½) and JUMPS at θ = 0 (0⁻ → 0, 0 → 1): the seam of the side maps is the half-plane z = 0, x > 0 of object space."""
    return np.where(theta < 0, -theta / (2 * GL_PI), 1 - theta / (2 * GL_PI))


def uv_map(kind, p, rep, size):
    """The uv maps of frag:1299-1398 for object-space points p → (uv scaled by (repeatU, repeatV), margin).  size = (columns, rows)
    of the texture; margin: how far (in texels of that texture) p lies from the nearest place where uv jumps — a cube-face tie
    (`m == absP.x`, …), a cap test |y ± 0.5| < TEXTURE_EPS, the side maps' seam at θ = 0 and their axis (atan(0, 0)), the sphere's
    poles.  Within the side maps, p at object-space distance δ from the seam is |θ|/2π·|repeatU|·columns texels from it."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    rate = max(abs(rep[0]) * size[0], abs(rep[1]) * size[1])  # texels per object-space unit of the planar maps
    theta = np.arctan2(z, x)
    rxz = np.sqrt(x * x + z * z)
    side_u = _u_from_theta(theta)
    side_m = np.minimum(np.abs(theta) / (2 * GL_PI) * abs(rep[0]) * size[0], rxz * rate)
    if kind == RM_CUBE:
        a = np.abs(p)
        m = np.max(a, -1)
        second = np.sort(a, -1)[:, 1]
        u = np.select([(m == a[:, 0]) & (x < 0), m == a[:, 0], m == a[:, 1]], [z + 0.5, -z + 0.5, x + 0.5], np.where(z < 0, -x + 0.5, x + 0.5))
        v = np.select([m == a[:, 0], (m == a[:, 1]) & (y < 0), m == a[:, 1]], [y + 0.5, z + 0.5, -z + 0.5], y + 0.5)
        margin = (m - second) * rate
    elif kind == RM_CONE:
        cap = np.abs(y + 0.5) < TEXTURE_EPS
        u = np.where(cap, x + 0.5, side_u)
        v = np.where(cap, z + 0.5, y + 0.5)
        margin = np.minimum(np.abs(np.abs(y + 0.5) - TEXTURE_EPS) * rate, np.where(cap, np.inf, side_m))
    elif kind == RM_CYLINDER:
        top, bottom = np.abs(y - 0.5) < TEXTURE_EPS, np.abs(y + 0.5) < TEXTURE_EPS
        u = np.where(top | bottom, x + 0.5, side_u)
        v = np.where(top, -z + 0.5, np.where(bottom, z + 0.5, y + 0.5))
        margin = np.minimum(np.minimum(np.abs(np.abs(y - 0.5) - TEXTURE_EPS), np.abs(np.abs(y + 0.5) - TEXTURE_EPS)) * rate,
                            np.where(top | bottom, np.inf, side_m))
    elif kind == RM_SPHERE:
        # v = asin(y / 0.5)/π + ½.  A hit point lies within SURFACE_DIST of the surface, so |y / 0.5| can exceed 1 near a pole,
        # where GLSL's asin is undefined: the argument is clamped to [−1, 1] (asin saturates at ±π/2).  The pole rule `v == 0 ||
        # v == 1 ⇒ u = ½` holds in binary32 exactly where that argument reaches ±1 (π/2 over the binary32 PI is ½ exactly there,
        # and asin of the next binary32 below 1 is 3e-4 short of π/2); in real arithmetic with the shader's PI it would never
        # hold.  So the rule is taken as |y| ≥ 0.5, and that boundary is one of the jumps of the margin.
        s_ = np.clip(y / 0.5, -1.0, 1.0)
        pole = np.abs(y) >= 0.5
        v = np.where(pole, np.where(y > 0, 1.0, 0.0), np.arcsin(s_) / GL_PI + 0.5)
        u = np.where(pole, 0.5, side_u)
        margin = np.minimum(np.abs(np.abs(y) - 0.5) * rate, np.where(pole, np.inf, side_m))
        return np.stack([u * rep[0], v * rep[1]], -1), margin, pole
    else:
        raise ValueError(f"object type {kind} has no uv map (UB4 / rm_render_ex: rejected)")
    return np.stack([u * rep[0], v * rep[1]], -1), margin, np.zeros(len(p), bool)


def get_diffuse(objs, textures, k, p, kd):
    """getDiffuse (frag:1746-1781) at world points p of objects k → (rgb, margin in texels — inf for untextured objects —, whether
    the sphere's pole rule decided u)."""
    rgb = kd * objs["cDiffuse"][k]
    margin, pole = np.full(len(p), np.inf), np.zeros(len(p), bool)
    for j in np.unique(k):
        tl = int(objs["texLoc"][j])
        if tl == -1:
            continue
        sel = k == j
        M = objs["invModel"][j]
        po = p[sel] @ M[:3, :3].T + M[:3, 3]                     # vec3(invModel · vec4(p, 1))
        img = textures[tl]
        uv, m, pl = uv_map(int(objs["type"][j]), po, (objs["repeatU"][j], objs["repeatV"][j]), (img.shape[1], img.shape[0]))
        tex = sample_rgba8(img, uv[:, 0], uv[:, 1], REPEAT)[:, :3]
        bl = objs["blend"][j]
        rgb[sel] = (1.0 - bl) * kd * objs["cDiffuse"][j] + bl * tex
        margin[sel], pole[sel] = m, pl
    return rgb, margin, pole


def integrate_edge_vec(v1, v2):  # frag:349-361
    x = _dot(v1, v2)
    y = np.abs(x)
    a = 0.8543985 + (0.4965155 + 0.0145206 * y) * y
    b = 3.4175940 + (4.1616724 + y) * y
    v = a / b
    ts = np.where(x > 0.0, v, 0.5 / np.sqrt(np.maximum(1.0 - x * x, 1e-7)) - v)
    return np.cross(v1, v2) * ts[:, None]


def ltc_evaluate(N, V, P, Minv, points, two_sided, ltc2):
    """LTC_Evaluate (frag:368-424) → (sum, margin).  Minv: (n, 3, 3) or (3, 3), numpy row-major.  UB11: len == 0 ⇒
    z = 0.  `behind` is dot(points[0] − P, (p1 − p0) × (p3 − p0)) < 0; margin = |cos| of that angle (the jump of `behind`, which
    flips z and, for a one-sided light, zeroes the term)."""
    T1 = _normalize(V - N * _dot(V, N)[:, None])
    T2 = np.cross(N, T1)
    B = np.stack([T1, T2, N], 1)                  # transpose(mat3(T1, T2, N)): its ROWS are T1, T2, N
    M = np.matmul(Minv, B)
    L = [_normalize(np.einsum("nij,nj->ni", M, pt - P)) for pt in points]
    d0 = points[0] - P
    ln = np.cross(points[1] - points[0], points[3] - points[0])
    cosb = _dot(d0, np.broadcast_to(ln, d0.shape))
    behind = cosb < 0.0
    margin = np.abs(cosb) / (np.sqrt(_dot(d0, d0)) * np.sqrt(ln @ ln))
    vsum = integrate_edge_vec(L[0], L[1]) + integrate_edge_vec(L[1], L[2]) + integrate_edge_vec(L[2], L[3]) + integrate_edge_vec(L[3], L[0])
    ln_ = np.sqrt(_dot(vsum, vsum))
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.where(ln_ == 0.0, 0.0, vsum[:, 2] / ln_)
    z = np.where(behind, -z, z)
    scale = sample_rgba8(ltc2, (z * 0.5 + 0.5) * LUT_SCALE + LUT_BIAS, ln_ * LUT_SCALE + LUT_BIAS, CLAMP_TO_EDGE)[:, 3]
    s = ln_ * scale
    return np.where(~behind & (not two_sided), 0.0, s), margin


def get_area_light(N, V, P, li, cS, dif, ltc):
    """getAreaLight (frag:1794-1822) → (colour, margin of the `behind` tests).  The LTC fetches are GL_LINEAR with CLAMP_TO_EDGE at
    uv·LUT_SCALE + LUT_BIAS (UB8).  Minv = mat3(col0, col1, col2) is built from COLUMNS (t1.x, 0, t1.y), (0, 1, 0), (t1.z, 0, t1.w)."""
    ltc1, ltc2 = ltc
    dnv = np.clip(_dot(N, V), 0.0, 1.0)
    uu = np.full(len(N), LUT_BIAS)                 # uv = (0, sqrt(1 − N·V))·LUT_SCALE + LUT_BIAS
    vv = np.sqrt(1.0 - dnv) * LUT_SCALE + LUT_BIAS
    t1 = sample_rgba8(ltc1, uu, vv, CLAMP_TO_EDGE)
    t2 = sample_rgba8(ltc2, uu, vv, CLAMP_TO_EDGE)
    Minv = np.zeros((len(N), 3, 3))
    Minv[:, :, 0] = np.stack([t1[:, 0], np.zeros(len(N)), t1[:, 1]], -1)   # column 0
    Minv[:, 1, 1] = 1.0                                                      # column 1
    Minv[:, :, 2] = np.stack([t1[:, 2], np.zeros(len(N)), t1[:, 3]], -1)   # column 2
    pts = li["points"]
    diffuse, m1 = ltc_evaluate(N, V, P, np.broadcast_to(np.eye(3), Minv.shape), pts, li["twoSided"], ltc2)
    specular, m2 = ltc_evaluate(N, V, P, Minv, pts, li["twoSided"], ltc2)
    spec = specular[:, None] * (cS * t2[:, 0:1] + (li["intensity"] - cS) * t2[:, 1:2])
    return li["color"] * (spec + dif * diffuse[:, None]), np.minimum(m1, m2)


def _march(sd, ro, rd, end, max_steps):
    """raymarch (frag:1453-1484, side = +1) → (hit, depth rayDepth − minD, intersectObj, margin = min | |d| − SURFACE_DIST |)."""
    n = len(ro)
    t, d = np.zeros(n), np.full(n, 1000000.0)
    obj, margin = np.full(n, -1), np.full(n, np.inf)
    idx = np.arange(n)
    for _ in range(max_steps):
        if len(idx) == 0:
            break
        dd, tr = sd(ro[idx] + rd[idx] * t[idx, None])
        d[idx], obj[idx] = dd, tr[:, 0].astype(int)
        margin[idx] = np.minimum(margin[idx], np.abs(np.abs(dd) - SURFACE_DIST))
        go = ~((np.abs(dd) < SURFACE_DIST) | (t[idx] > end))
        t[idx[go]] += dd[go]
        idx = idx[go]
    hit = np.abs(d) < SURFACE_DIST
    return hit, t - d, np.where(hit, obj, -1), margin


class _Frame:
    """What render() reads besides its arguments: the scene, the lights, the samplers, the background."""

    def __init__(self, tables, settings, resources):
        res = resources or {}
        self.settings, self.g = settings, tables.globals_
        self.far = float(tables.camera.initialFar)
        objs, o_ = [], {k: [] for k in ("cAmbient", "cDiffuse", "cSpecular", "cReflective", "cTransparent", "shininess", "ior", "texLoc",
                                       "repeatU", "repeatV", "blend", "type", "invModel", "isEmissive", "color", "lightIdx")}
        for i in range(tables.num_objects):
            o = tables.objects[i]
            assert o.type in Table.SDF
            M = np.array(list(o.invModel), np.float64).reshape(4, 4).T
            objs.append((o.type, M, o.scaleFactor))
            for k in ("cAmbient", "cDiffuse", "cSpecular", "cReflective", "cTransparent", "color"):
                o_[k].append(list(getattr(o, k)))
            for k in ("shininess", "ior", "repeatU", "repeatV", "blend"):
                o_[k].append(float(getattr(o, k)))
            for k in ("texLoc", "type", "isEmissive", "lightIdx"):
                o_[k].append(int(getattr(o, k)))
            o_["invModel"].append(M)
            if o.texLoc != -1:
                assert o.type in (RM_CUBE, RM_CONE, RM_CYLINDER, RM_SPHERE), "no uv map for this type (UB4)"
                assert res.get("textures") is not None and o.texLoc < len(res["textures"])
        self.objs = {k: np.array(v) for k, v in o_.items()}
        self.objs["lightIdx_table"] = self.objs["lightIdx"]
        self.lights = []
        for i in range(tables.num_lights):
            li = tables.lights[i]
            assert li.type in (RM_LIGHT_DIRECTIONAL, RM_LIGHT_POINT, RM_LIGHT_SPOT, RM_LIGHT_AREA)
            self.lights.append({"type": li.type, "dir": np.array(list(li.dir), np.float64), "pos": np.array(list(li.pos), np.float64),
                                "func": np.array(list(li.func), np.float64), "color": np.array(list(li.color), np.float64),
                                "angle": float(li.angle), "penumbra": float(li.penumbra), "intensity": float(li.intensity),
                                "twoSided": bool(li.twoSided), "points": [np.array(list(li.points[c]), np.float64) for c in range(4)]})
        self.textures = res.get("textures")
        self.skybox = res.get("skybox") if settings.enableSkyBox else None
        assert not settings.enableSkyBox or self.skybox is not None
        self.ltc = (res.get("ltc1"), res.get("ltc2"))
        assert all(li["type"] != RM_LIGHT_AREA for li in self.lights) or self.ltc[0] is not None
        f = settings.features
        assert not f & (RM_FEAT_SKY_BACKGROUND | RM_FEAT_NIGHTSKY_BACKGROUND | RM_FEAT_CLOUD | RM_FEAT_TERRAIN | RM_FEAT_SEA), \
            "procedural layers are not transcribed"
        self.bg = np.zeros(3)                      # setScene, frag:2414-2420: no background #define ⇒ (0, 0, 0)
        if f & RM_FEAT_WHITE_BACKGROUND:
            self.bg = np.ones(3)
        if f & RM_FEAT_DARK_BACKGROUND:
            self.bg = np.zeros(3)
        self.sd = Table(objs)
        self.njitter = 0.0

    def rays(self, ro, rd, margins):
        """render() (frag:2318-2375) for a batch of rays → (rgb, isEnv, isAL, hit point, shading normal, object).  `margins` (dict
        of per-ray arrays: "tex", "geom", "cos", "pole") is lowered in place by every decision of these rays that jumps."""
        n, s = len(ro), self.settings
        rgb = np.broadcast_to(self.bg, (n, 3)).copy()
        P, N, K = np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, -1)
        hit, depth, obj, gm = _march(self.sd, ro, rd, self.far, s.maxSteps)
        margins["geom"] = np.minimum(margins["geom"], gm)
        if self.skybox is not None and (~hit).any():              # frag:2327
            sky, cm = sample_cube(self.skybox, rd[~hit])
            rgb[~hit] = sky
            margins["tex"][~hit] = np.minimum(margins["tex"][~hit], cm)
        emis = hit & (self.objs["isEmissive"][np.maximum(obj, 0)] != 0)
        rgb[emis] = self.objs["color"][obj[emis]]                 # isAL: obj.color, frag:2339-2342
        sh = hit & ~emis
        if sh.any():
            p = ro[sh] + rd[sh] * depth[sh, None]
            pn = get_normal(self.sd, p)
            if s.features & RM_FEAT_PERLIN_BUMP:
                pn = bump_normal(pn, p)
            if self.njitter:
                axis = np.random.default_rng(len(p)).normal(size=p.shape)
                pn = _normalize(pn + self.njitter * _normalize(np.cross(pn, axis)))
            k = obj[sh]
            m = {key: self.objs[key][k] for key in ("cAmbient", "cDiffuse", "cSpecular", "shininess")}
            m["lightIdx_table"] = self.objs["lightIdx"]
            g = self.g
            dif, tm, pl = get_diffuse(self.objs, self.textures, k, p, g.kd)
            sub = {"geom": np.full(len(p), np.inf), "cos": np.full(len(p), np.inf)}
            rgb[sh] = get_phong_table(self.sd, pn, m, self.lights, (g.ka, g.kd, g.ks), p, rd[sh], self.far, s, k=k, dif=dif,
                                      ltc=self.ltc, margins=sub)
            margins["tex"][sh] = np.minimum(margins["tex"][sh], tm)
            margins["pole"][sh] = np.where(pl, 0.0, margins["pole"][sh])
            margins["geom"][sh] = np.minimum(margins["geom"][sh], sub["geom"])
            margins["cos"][sh] = np.minimum(margins["cos"][sh], sub["cos"])
            P[sh], N[sh], K[sh] = p, pn, k
        return rgb, ~hit, emis, P, N, K


def render_frame_table(tables, settings, W, H, resources=None, diag=False, jitter=None):
    """fragColor of every pixel of a table of primitives (H, W, 4) float64 and the hit mask: directional, point, spot and AREA
    lights (LTC, frag:349-424, 1794-1822, 1884-1905), objects textured through the uv maps and getDiffuse's blend, the emissive
    rectangles of area lights (isAL), a miss coloured by the white or dark background or by the sky box (frag:2323-2327); main's
    reflection loop (frag:2491-2524: the FIRST hit's cReflective filters every bounce) and its two-interface refraction
    (frag:2526-2570) when they are enabled.  `resources`: dict with textures= (list, slot = texLoc), skybox= (six faces +X…−Z),
    ltc1= / ltc2= (uint8 64×64×4), all in upload order.
    diag=True adds a dict: "bright" (BrightColor, setBrightness frag:1938-1946), "obj" (primary object, −1 on a miss) and the
    per-pixel margins — "tex" (texels from a uv jump, a cube-face edge), "geom" (world units between some march's |d| and
    SURFACE_DIST: silhouettes and shadow edges), "cos" (N·L from 0.005, |cos| of an LTC `behind` test), "lum" (|luminance − 1|,
    the jump of setBrightness), "pole" (0 where some shading point took the sphere's pole rule — which the C arbiter, comparing
    a binary64 v with 1, never takes: see uv_map).
    jitter = (a, b): turn every primary ray by a and every shading normal by b radians about fixed pseudo-random axes — the frame
    seen through rays a few binary32 ulps off and with normals as noisy as getNormal's four-tap difference is in binary32 (an ulp
    of a distance over e = 2.9e-4: ≈ 2e-4); |frame − jittered frame| measures how ill-conditioned a pixel is (grazing hits, shadow
    rays that skim an edge, mirrors), which a binary32 evaluation amplifies alike."""
    assert not tables.globals_.isTwoD
    fr = _Frame(tables, settings, resources)
    sd, far, gl = fr.sd, fr.far, fr.g
    inv_pv = np.array(list(tables.camera.invProjView), np.float64).reshape(4, 4).T
    ys, xs = np.mgrid[0:H, 0:W]
    ndc = np.stack([(xs.ravel() + 0.5) / W * 2.0 - 1.0, (ys.ravel() + 0.5) / H * 2.0 - 1.0], -1)
    near = np.concatenate([ndc, np.full((len(ndc), 1), -1.0), np.ones((len(ndc), 1))], -1) @ inv_pv.T
    farc = np.concatenate([ndc, np.ones((len(ndc), 1)), np.ones((len(ndc), 1))], -1) @ inv_pv.T
    ro = near[:, :3] / near[:, 3:]
    rd = _normalize(farc[:, :3] / farc[:, 3:] - ro)
    if jitter:
        axis = np.random.default_rng(12345).normal(size=(len(rd), 3))
        rd = _normalize(rd + jitter[0] * _normalize(np.cross(rd, axis)))
        fr.njitter = jitter[1]
    n = len(ndc)
    mg = {"tex": np.full(n, np.inf), "geom": np.full(n, np.inf), "cos": np.full(n, np.inf), "pole": np.full(n, np.inf)}
    out = np.ones((n, 4))
    rgb, is_env, is_al, P, N, K = fr.rays(ro, rd, mg)
    out[:, :3] = rgb
    # UB5: an emissive primary hit leaves `info` unset; main reads objects[−1] — zeros — so no reflection / refraction follows
    prim = ~is_env & ~is_al
    if settings.enableReflection:  # frag:2491-2524
        c_refl = fr.objs["cReflective"][np.maximum(K, 0)]
        idx = np.nonzero(prim & (np.sqrt(_dot(c_refl, c_refl)) != 0.0))[0]
        p, nn, d, cr = P[idx], N[idx], rd[idx], c_refl[idx]
        fil = np.ones((len(idx), 3))
        for _ in range(settings.numReflection):
            if len(idx) == 0:
                break
            r = d - 2.0 * _dot(nn, d)[:, None] * nn
            fil = fil * cr
            sub = {k: v[idx] for k, v in mg.items()}
            rgb2, env, al, P2, N2, _k2 = fr.rays(p + r * SURFACE_DIST * 3.0, r, sub)
            for k in mg:
                mg[k][idx] = sub[k]
            out[idx, :3] += gl.ks * fil * rgb2
            out[idx, 3] += 1.0
            # an emissive hit inside the loop leaves `info` as it was (UB5: the stale info is reused as written)
            P2, N2, r = np.where(al[:, None], p, P2), np.where(al[:, None], nn, N2), np.where(al[:, None], d, r)
            go = ~env
            idx, p, nn, d, cr, fil = idx[go], P2[go], N2[go], r[go], cr[go], fil[go]
    if settings.enableRefraction:  # frag:2526-2570: two interfaces, air → medium → air, from the PRIMARY hit (oi)
        k0 = np.maximum(K, 0)
        c_refr = fr.objs["cTransparent"][k0]
        idx = np.nonzero(prim & (np.sqrt(_dot(c_refr, c_refr)) != 0.0))[0]
        if len(idx):
            ior, ct = fr.objs["ior"][k0][idx], c_refr[idx]
            rd_in = _refract(rd[idx], N[idx], 1.0 / ior)
            p_enter = P[idx] - N[idx] * SURFACE_DIST * 3.0
            d_in = _raymarch_depth(sd, p_enter, rd_in, far, settings.maxSteps, side=-1.0)  # INSIDE; UB2: the depth travelled on a miss
            p_exit = p_enter + rd_in * d_in[:, None]
            n_exit = -get_normal(sd, p_exit)
            rd_out = _refract(rd_in, n_exit, ior)
            ok = np.sqrt(_dot(rd_out, rd_out)) != 0.0  # otherwise total internal reflection: refr = vec4(0)
            if ok.any():
                j = idx[ok]
                sub = {k: v[j] for k, v in mg.items()}
                rgb3, _e, _a, _p, _n, _k = fr.rays((p_exit - n_exit * SURFACE_DIST * 5.0)[ok], rd_out[ok], sub)
                for k in mg:
                    mg[k][j] = sub[k]
                out[j, :3] += gl.kt * ct[ok] * rgb3
                out[j, 3] += 1.0
    if not diag:
        return out.reshape(H, W, 4), (~is_env).reshape(H, W)
    lum = out[:, :3] @ BRIGHT_FILTER                       # setBrightness(col), frag:1938-1946; a miss: (0, 0, 0, 1), frag:2462
    bright = np.zeros((n, 4))
    bright[:, 3] = 1.0
    on = ~is_env & (lum > 1.0)
    bright[on, :3] = out[on, :3]
    info = {"bright": bright.reshape(H, W, 4), "obj": np.where(is_env, -1, K).reshape(H, W),
            "lum": np.where(is_env, np.inf, np.abs(lum - 1.0)).reshape(H, W)}
    info.update({k: v.reshape(H, W) for k, v in mg.items()})
    return out.reshape(H, W, 4), (~is_env).reshape(H, W), info


# ---------------------------------------------------------------------------------------------- the G-buffer (rm_render_gbuffer)
def gbuffer_frame(tables, settings, W, H, shift=0.0, wobble=None):
    """What the primary ray of every pixel hits, from the definition in include/raymarcher_amd.h (rm_render_gbuffer) and the shader
    text: main's first render() call up to the normal it hands getPhong (frag:2388-2392, 2443, 2318-2337) → float64 (normal (H, W, 3),
    depth (H, W), object_id (H, W), position (H, W, 4), geom_margin (H, W)), row 0 = bottom.
    The primary ray of a pixel is computed at that pixel from invProjView (raymarch.vert:13-25 at the pixel centre; nothing is
    interpolated from corners).  A table of one Mandelbulb or one Menger sponge marches through `raymarch` with Bulb / Menger, any
    other table (Table's primitives and the Sierpinski; an empty one too) through `_march`, both to initialFar with the call's
    maxSteps.  A hit: object_id is the march's index (an emissive rectangle reports ITSELF: nothing here reads isEmissive), depth =
    rayDepth − minD, p = ro + rd·depth, n = get_normal(p), then bump_normal(n, p) when RM_FEAT_PERLIN_BUMP is set; position = (p, 1).
    A miss: n = (0, 0, 0), depth = initialFar, object_id = −1, position = (0, 0, 0, 0).
    geom_margin: min over the march's evaluations of | |d| − SURFACE_DIST | — how far the nearest stopping test was from flipping
    (`raymarch` keeps no margin, so the fractals' comes from a second pass through `_march`, which must reproduce hit and depth).
    shift: evaluate the normal at p + rd·shift instead of p (depth and position stay those of p) — how much of a normal's error
    a hit point that is off by one stopping step along the ray explains.
    wobble=(δ, tol) appends a bool (H, W), `unstable`: the same march started δ further along the ray, or δ nearer, hits another
    object (or none), or ends — hit or miss, the depth the march reports — more than tol from where this one ends.  The march is the iteration t ← t + d(t).  About a surface crossed at
    angle θ, where d' = −k·cos θ, its derivative is 1 − k·cos θ; k = 1 for a true distance, but the ABI accepts any scaleFactor, and
    with one above the smallest scale of the model (or a sheared model) k·cos θ can exceed 2.  Then the iteration is no contraction:
    the ray bounces about the surface, every step multiplies a rounding difference, and where — or whether, within maxSteps — it
    lands inside SURFACE_DIST is decided by the last bit of the first step.  geom_margin, the distance of THIS trajectory's stopping
    tests from flipping, does not see that; with δ one binary32 ulp of the depth, such a pixel is defined by its binary32
    evaluation alone."""
    assert not tables.globals_.isTwoD
    assert not settings.features & (RM_FEAT_CLOUD | RM_FEAT_TERRAIN | RM_FEAT_SEA)
    gl, n_obj = tables.globals_, tables.num_objects
    far = float(tables.camera.initialFar)
    inv_pv = np.array(list(tables.camera.invProjView), np.float64).reshape(4, 4).T  # column-major storage
    ys, xs = np.mgrid[0:H, 0:W]
    ndc = np.stack([(xs.ravel() + 0.5) / W * 2.0 - 1.0, (ys.ravel() + 0.5) / H * 2.0 - 1.0], -1)
    near = np.concatenate([ndc, np.full((len(ndc), 1), -1.0), np.ones((len(ndc), 1))], -1) @ inv_pv.T
    farc = np.concatenate([ndc, np.ones((len(ndc), 1)), np.ones((len(ndc), 1))], -1) @ inv_pv.T
    ro = near[:, :3] / near[:, 3:]                      # setScene, frag:2388-2392
    rd = _normalize(farc[:, :3] / farc[:, 3:] - ro)

    def inv_model(o):
        return np.array(list(o.invModel), np.float64).reshape(4, 4).T
    fractal = n_obj == 1 and tables.objects[0].type in (RM_MANDELBULB, RM_MENGERSPONGE)
    if fractal:
        o = tables.objects[0]
        if o.type == RM_MANDELBULB:
            sd = Bulb(inv_model(o), o.scaleFactor, gl.power, settings.fractalIters, (gl.juliaSeed[0], gl.juliaSeed[1]))
        else:
            sd = Menger(inv_model(o), o.scaleFactor, settings.mengerLevels, gl.iTime)
        hit, depth, _trap = raymarch(sd, ro, rd, far, settings.maxSteps)
        hit2, depth2, _obj, margin = _march(sd, ro, rd, far, settings.maxSteps)
        assert (hit2 == hit).all() and (depth2[hit] == depth[hit]).all()
        obj = np.where(hit, 0, -1)
    else:
        sd = Table([(tables.objects[i].type, inv_model(tables.objects[i]), tables.objects[i].scaleFactor) for i in range(n_obj)])
        hit, depth, obj, margin = _march(sd, ro, rd, far, settings.maxSteps)
    n = len(ro)
    N, P, D = np.zeros((n, 3)), np.zeros((n, 4)), np.full(n, far)
    if hit.any():
        p = ro[hit] + rd[hit] * depth[hit, None]         # frag:2333
        q = p + rd[hit] * shift
        pn = get_normal(sd, q)
        if settings.features & RM_FEAT_PERLIN_BUMP:      # frag:2334-2336
            pn = bump_normal(pn, q)
        N[hit], D[hit] = pn, depth[hit]
        P[hit, :3], P[hit, 3] = p, 1.0
    res = (N.reshape(H, W, 3), D.reshape(H, W), np.where(hit, obj, -1).astype(np.float64).reshape(H, W), P.reshape(H, W, 4),
           margin.reshape(H, W))
    if wobble is None:
        return res
    unstable = np.zeros(n, bool)
    for dt in (wobble[0], -wobble[0]):
        hit_w, depth_w, obj_w, _m = _march(sd, ro + rd * dt, rd, far, settings.maxSteps)
        if fractal:
            obj_w = np.zeros(n, int)   # the fractal classes carry their trap where a table carries the index
        unstable |= (hit_w != hit) | (hit & (np.where(hit_w, obj_w, -1) != np.where(hit, obj, -1))) | (np.abs(depth_w + dt - depth) > wobble[1])
    return res + (unstable.reshape(H, W),)
