"""Host-side driver of the C-ABI: scene tables, camera, row-range / row-tile renders into torch tensors.

Mirrors the reference's scene surface — RayMarchScene::initScene/getShapes/getLights/getCamera/
getGlobalData (src/raymarch/raymarchscene.h:12-90) and Realtime::rayMarch / saveViewportImage
(src/realtimerender.cpp:53-87, src/realtime.cpp:284-350) — on top of rm_scene_*, rm_camera_build,
rm_render*, rm_frame_to_rgba8 and rm_write_png.
"""
import ctypes as C
import threading
from dataclasses import dataclass

from . import abi
from ._lib import RaymarcherError, check, lib


@dataclass
class SceneTables:
    """The uniform tables one frame needs (what configure*Uniforms upload, realtimerender.cpp:596-811)."""
    camera: abi.RmCamera
    objects: C.Array
    num_objects: int
    lights: C.Array
    num_lights: int
    globals_: abi.RmGlobals
    textures: list = None  # host uint8 arrays (H, W, 4), rows bottom-up, indexed by RmObject.texLoc
    noise: object = None   # uint8 (H, W, 4): the `noise` sampler of NIGHTSKY_BACKGROUND / SEA (noise_texture_1.png, mirrored)
    skybox: list = None    # six uint8 (H, W, 4) cube-map faces +X,-X,+Y,-Y,+Z,-Z as uploaded (mirrored at load)
    ltc1: object = None    # uint8 (64, 64, 4) LTC tables of the area lights (ltc_quantise of the float tables)
    ltc2: object = None

    def args(self, settings):
        return (C.byref(self.camera), self.objects, self.num_objects, self.lights, self.num_lights,
                C.byref(self.globals_), C.byref(settings))


def load_image(path, flip_vertical=True):
    """rm_image_load → numpy uint8 (H, W, 4); flip_vertical=True gives the bottom-up rows the renderer samples
    (QImage::mirrored at load, raymarchscene.cpp:208)."""
    import numpy as np
    px, w, h = C.c_void_p(), C.c_int(), C.c_int()
    check(lib().rm_image_load(str(path).encode(), 1 if flip_vertical else 0, C.byref(px), C.byref(w), C.byref(h)))
    try:
        arr = np.ctypeslib.as_array(C.cast(px, C.POINTER(C.c_uint8)), shape=(h.value, w.value, 4)).copy()
    finally:
        lib().rm_image_free(px)
    return arr


def ltc_quantise(table):
    """Float RGBA table → the 8-bit texels the reference's glTexImage2D(GL_RGBA, …, GL_FLOAT, LTC) upload leaves
    (realtimerender.cpp:908, 925)."""
    import numpy as np
    t = np.ascontiguousarray(table, dtype=np.float32).reshape(-1, 4)
    out = np.empty(t.shape, dtype=np.uint8)
    lib().rm_ltc_quantise(C.c_void_p(t.ctypes.data), C.c_void_p(out.ctypes.data), t.shape[0])
    return out.reshape(np.shape(table))


def build_camera(pos, look, up, height_angle_rad, W, H, near=0.1, far=100.0):
    """Camera::initializeCamera + configureCameraUniforms via rm_camera_build (camera.cpp:8-133)."""
    cd = abi.RmCameraData()
    for i in range(3):
        cd.pos[i], cd.look[i], cd.up[i] = pos[i], look[i], up[i]
    cd.pos[3], cd.look[3], cd.up[3] = 1.0, 0.0, 0.0
    cd.heightAngle = height_angle_rad
    cam = abi.RmCamera()
    view = (C.c_float * 16)()
    proj = (C.c_float * 16)()
    check(lib().rm_camera_build(C.byref(cd), W, H, near, far, view, proj, C.byref(cam)))
    return cam, list(view), list(proj)


class Scene:
    """A parsed scenefile (SceneParser::parse + RayMarchScene::initScene)."""

    def __init__(self, path=None, text=None):
        self._h = C.c_void_p()
        L = lib()
        if path is not None:
            check(L.rm_scene_load(str(path).encode(), C.byref(self._h)))
        elif text is not None:
            check(L.rm_scene_load_string(text.encode(), C.byref(self._h)))
        else:
            raise ValueError("path or text required")

    def close(self):
        if self._h:
            lib().rm_scene_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def num_objects(self):
        return lib().rm_scene_num_objects(self._h)

    @property
    def num_lights(self):
        return lib().rm_scene_num_lights(self._h)

    def camera_data(self):
        cd = abi.RmCameraData()
        check(lib().rm_scene_camera_data(self._h, C.byref(cd)))
        return cd

    def lens(self):
        """rm_scene_camera_lens: the scenefile's (aperture, focalLength), which this library reads as the lens radius and the
        focus distance of lens_cameras, in world units; 0.0 for a field the file does not have."""
        a, f = C.c_float(), C.c_float()
        check(lib().rm_scene_camera_lens(self._h, C.byref(a), C.byref(f)))
        return a.value, f.value

    def texture_of(self, i):
        t = lib().rm_scene_object_texture(self._h, i)
        return t.decode() if t else None

    def tables(self, W, H, near=0.1, far=100.0, host_settings=None, load_textures=True):
        """Copy the tables out (so they outlive the handle) and build the camera for a W×H frame.
        load_textures=False leaves `textures` empty for the caller to fill (slot i = RmObject.texLoc i)."""
        L = lib()
        no, nl = self.num_objects, self.num_lights
        objs = (abi.RmObject * max(no, 1))()
        lights = (abi.RmLight * max(nl, 1))()
        po, pl = L.rm_scene_objects(self._h), L.rm_scene_lights(self._h)
        for i in range(no):
            C.memmove(C.byref(objs[i]), C.byref(po[i]), C.sizeof(abi.RmObject))
        for i in range(nl):
            C.memmove(C.byref(lights[i]), C.byref(pl[i]), C.sizeof(abi.RmLight))
        g = abi.RmGlobals()
        hs = host_settings
        check(L.rm_scene_globals(self._h, C.byref(hs) if hs is not None else None, C.byref(g)))
        cd = self.camera_data()
        cam = abi.RmCamera()
        check(L.rm_camera_build(C.byref(cd), W, H, near, far, None, None, C.byref(cam)))
        # texture slots in texLoc order (configureShapesUniforms binds them in first-use order, realtimerender.cpp:735-806)
        textures = {}
        for i in range(no if load_textures else 0):
            if objs[i].texLoc >= 0 and objs[i].texLoc not in textures:
                try:
                    textures[objs[i].texLoc] = load_image(self.texture_of(i), flip_vertical=True)
                except RaymarcherError as e:
                    if e.status != abi.RM_ERR_IO:
                        raise
                    # a texture file that is not there: the reference prints "Failed to load in image", still creates the GL
                    # texture (initShapesTextures, realtimerender.cpp:266-303) and samples the incomplete texture, which
                    # reads (0,0,0,1) — a 1×1 black texel gives the same samples
                    import numpy as np
                    textures[objs[i].texLoc] = np.array([[[0, 0, 0, 255]]], dtype=np.uint8)
        tex_list = [textures[k] for k in sorted(textures)] if textures else None
        return SceneTables(cam, objs, no, lights, nl, g, tex_list)


def lens_cameras(camera_data, W, H, radius, focus, n, near=0.1, far=100.0):
    """rm_camera_lens_samples: the n cameras of a thin lens of `radius` focused at distance `focus` along the view direction of
    `camera_data` (an RmCameraData, e.g. Scene.camera_data()) → a list of n RmCamera for Renderer.render_accumulated.  The first
    is the pinhole camera itself."""
    n = int(n)
    if n < 1:
        raise ValueError(f"n = {n}: a lens needs at least one sample")
    out = (abi.RmCamera * n)()
    check(lib().rm_camera_lens_samples(C.byref(camera_data), W, H, near, far, radius, focus, n, out))
    cams = []
    for c in out:  # copies that own their memory, not views into the array
        cam = abi.RmCamera()
        C.memmove(C.byref(cam), C.byref(c), C.sizeof(abi.RmCamera))
        cams.append(cam)
    return cams


def shutter_globals(globals_, t_open, t_close, n):
    """n copies of the RmGlobals `globals_` with iTime at the midpoints of the n equal parts of the shutter interval
    [t_open, t_close] — t_open + (j + 0.5)·(t_close − t_open) / n, computed in float64 and rounded once — for
    Renderer.render_accumulated."""
    n = int(n)
    if n < 1:
        raise ValueError(f"n = {n}: a shutter interval needs at least one sample")
    t_open, t_close = float(t_open), float(t_close)
    out = []
    for j in range(n):
        g = abi.RmGlobals()
        C.memmove(C.byref(g), C.byref(globals_), C.sizeof(abi.RmGlobals))
        g.iTime = t_open + (j + 0.5) * (t_close - t_open) / n  # the c_float field rounds the float64 value once
        out.append(g)
    return out


def camera_rays(camera, W, H, pixels=None):
    """rm_camera_rays: the primary rays of `camera` (an RmCamera) for a W×H frame → float32 (n, 8) numpy array, one RmRay per row:
    (origin.xyz, tMax = the camera's initialFar, dir.xyz, 0).  pixels: None (every pixel, row-major, row 0 at the bottom, n = W·H)
    or n pairs (x, y).  Origin and dir are bit for bit what rm_render and rm_render_gbuffer use for that pixel, so
    Renderer.trace_rays on them gives the G-buffer's values.  A host function: it needs no GPU."""
    import numpy as np
    if pixels is None:
        xy, n = None, int(W) * int(H)
    else:
        xy = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1, 2)
        n = len(xy)
    out = np.zeros((n, 8), dtype=np.float32)
    check(lib().rm_camera_rays(C.byref(camera), W, H, xy.ctypes.data_as(C.POINTER(C.c_int32)) if xy is not None else None, n,
                               C.c_void_p(out.ctypes.data)))
    return out


def panorama_rays(position, W, H, forward=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0)):
    """The rays of a W×H equirectangular (360° × 180°) panorama seen from `position` → float32 (W·H, 8) numpy array of RmRay rows,
    row-major, row 0 at the bottom: (position, tMax = 0 (unread), dir, 0).  With u = (x + ½)/W, v = (y + ½)/H the angles are θ = (u −
    ½)·2π (0 = forward, positive to the right) and φ = (v − ½)·π (positive upwards); right = normalize(forward × up), up' = right ×
    forward, dir = cos φ·sin θ·right + sin φ·up' + cos φ·cos θ·normalize(forward).  Computed in float64 and rounded once to float32,
    so |dir| is 1 to within the rounding of its components.  A host function: it needs no GPU; Renderer.shade_rays takes the
    result."""
    import numpy as np
    f = np.asarray(forward, dtype=np.float64)
    f = f / np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, dtype=np.float64))
    if not np.linalg.norm(r) > 0.0:
        raise ValueError("forward and up are parallel")
    r = r / np.linalg.norm(r)
    u2 = np.cross(r, f)
    theta = ((np.arange(W, dtype=np.float64) + 0.5) / W - 0.5) * (2.0 * np.pi)
    phi = ((np.arange(H, dtype=np.float64) + 0.5) / H - 0.5) * np.pi
    cp, sp = np.cos(phi)[:, None, None], np.sin(phi)[:, None, None]
    ct, st = np.cos(theta)[None, :, None], np.sin(theta)[None, :, None]
    d = cp * st * r + sp * u2 + cp * ct * f
    out = np.zeros((H * W, 8), dtype=np.float32)
    out[:, 0:3] = np.asarray(position, dtype=np.float64)
    out[:, 4:7] = d.reshape(-1, 3)
    return out


def tile_order(W, H, tile=8):
    """The permutation (int64, W·H) that lists the pixels of a row-major W×H frame tile by tile, tile×tile pixels each, tiles in
    raster order and row-major inside a tile; the ragged tiles of the right and top edges keep the pixels they have.  rays[order]
    puts the rays that share a wave next to one another on the picture (64 consecutive rays are one 8×8 tile where the frame's
    sides are multiples of 8).  Measured: on the 4K Mandelbulb frame row-major rays cost 1.18 (trace_rays) to 1.23 (shade_rays) times
    as much; on a 1080p frame of primitives they were 6 % cheaper (profiles/shade_rays.md)."""
    import numpy as np
    y, x = np.divmod(np.arange(W * H, dtype=np.int64), W)
    tiles_x = (W + tile - 1) // tile
    key = ((y // tile) * tiles_x + x // tile) * (tile * tile) + (y % tile) * tile + x % tile
    return np.argsort(key, kind="stable")


def translated_objects(objs, index, offsets):
    """The stacked object tables of Renderer.render_animated for one moving object: table b is a copy of `objs` (a sequence or
    ctypes array of RmObject) whose entry `index` is moved by offsets[b] = (x, y, z) in world space through rm_object_translated
    → a ctypes array RmObject * (len(offsets)·len(objs)), table b at [b·len(objs) : (b + 1)·len(objs)].  Pass it as `objects`."""
    objs = list(objs)
    offsets = [tuple(float(v) for v in t) for t in offsets]
    if not objs or not all(isinstance(o, abi.RmObject) for o in objs):
        raise ValueError("objs must be a non-empty sequence of RmObject structs")
    if not isinstance(index, int) or isinstance(index, bool) or not 0 <= index < len(objs):
        raise ValueError(f"index = {index!r}: an entry of the {len(objs)}-object table")
    if not offsets or any(len(t) != 3 for t in offsets):
        raise ValueError("offsets must be a non-empty sequence of (x, y, z)")
    n = len(objs)
    out = (abi.RmObject * (len(offsets) * n))()
    for b, t in enumerate(offsets):
        for i, o in enumerate(objs):
            C.memmove(C.byref(out[b * n + i]), C.byref(o), C.sizeof(abi.RmObject))
        check(lib().rm_object_translated(C.byref(objs[index]), (C.c_float * 3)(*t), C.byref(out[b * n + index])))
    return out


def _stacked_tables(tables, what, struct, count, blocks):
    """The (array, number of tables) arguments of rm_render_animated for `tables` = None (one table: the scene's own, `count`
    entries) or the caller's per-block tables: a flat ctypes array / sequence of blocks·count structs, or a sequence of `blocks`
    sequences of `count` structs."""
    if tables is None:
        return None, 1
    rows = list(tables)
    if rows and not isinstance(rows[0], struct):
        if len(rows) != blocks or any(len(r) != count for r in rows):
            raise ValueError(f"{what} must have shape (blocks, {count}) = ({blocks}, {count})")
        rows = [e for r in rows for e in r]
    if len(rows) != blocks * count or not all(isinstance(e, struct) for e in rows):
        raise ValueError(f"{what} must hold blocks·count = {blocks}·{count} {struct.__name__} structs, one table per block")
    if isinstance(tables, C.Array) and tables._type_ is struct:
        return tables, blocks
    return (struct * max(len(rows), 1))(*rows), blocks


def batch_arrays(cameras, globals_):
    """The ctypes arrays of rm_render_batch: (RmCamera * N, RmGlobals * 1 or N).  globals_ is one RmGlobals (shared by every
    frame) or a sequence of N; raises ValueError on any other length or element type."""
    cameras = list(cameras)
    if not all(isinstance(c, abi.RmCamera) for c in cameras):
        raise ValueError("cameras must be RmCamera structs (build_camera(...)[0])")
    if len(cameras) > abi.RM_MAX_BATCH_FRAMES:
        raise ValueError(f"{len(cameras)} cameras: at most RM_MAX_BATCH_FRAMES = {abi.RM_MAX_BATCH_FRAMES} frames per batch")
    globs = [globals_] if isinstance(globals_, abi.RmGlobals) else list(globals_)
    if not all(isinstance(g, abi.RmGlobals) for g in globs):
        raise ValueError("globals_ must be an RmGlobals or a sequence of them")
    if len(globs) != len(cameras) and len(globs) != 1:
        raise ValueError(f"{len(globs)} globals for {len(cameras)} cameras: pass one, or one per camera")
    return (abi.RmCamera * max(len(cameras), 1))(*cameras), (abi.RmGlobals * len(globs))(*globs)


def post_array(post, n):
    """The ctypes array of rm_post_process_batch: RmPostSettings * 1 or N.  post is one RmPostSettings (every frame) or a sequence
    of n; the enable flags must be the same in every entry (only exposure may differ).  Raises ValueError otherwise."""
    posts = [post] if isinstance(post, abi.RmPostSettings) else list(post)
    if not all(isinstance(p, abi.RmPostSettings) for p in posts):
        raise ValueError("post must be an RmPostSettings or a sequence of them")
    if len(posts) != n and len(posts) != 1:
        raise ValueError(f"{len(posts)} post settings for {n} frames: pass one, or one per frame")
    if len({(p.enableFXAA, p.enableGammaCorrection, p.enableHDR, p.enableBloom) for p in posts}) > 1:
        raise ValueError("the enable flags must be the same for every frame; only exposure may differ")
    return (abi.RmPostSettings * len(posts))(*posts)


def save_png_sequence(images8, pattern):
    """Write the (N, H, W, 4) uint8 images (top row first, as to_rgba8_batch / render_sequence return them) with rm_write_png,
    image i to pattern.format(i), e.g. pattern="frame_{:04d}.png".  Returns the paths written."""
    import numpy as np
    imgs = images8.cpu().numpy() if hasattr(images8, "cpu") else np.asarray(images8)
    if imgs.ndim != 4 or imgs.shape[-1] != 4 or imgs.dtype != np.uint8:
        raise ValueError("images8 must be uint8 of shape (N, H, W, 4)")
    paths = []
    for i, img in enumerate(imgs):
        img = np.ascontiguousarray(img)
        path = pattern.format(i)
        check(lib().rm_write_png(str(path).encode(), C.c_void_p(img.ctypes.data), img.shape[1], img.shape[0]))
        paths.append(path)
    return paths


def _vec3(v, name):
    """Three floats as the (C.c_float * 3) the lattice calls take."""
    vals = [float(x) for x in v]
    if len(vals) != 3:
        raise ValueError(f"{name} must have three components")
    return (C.c_float * 3)(*vals)


def mesh_bounds(tables, margin=0.0):
    """The axis-aligned box (lo, hi), two float32 arrays of 3, that holds every surface of the object table, widened by `margin` on
    every side: the box of rm_debug_cull_bounds where the launcher stages one, else the box around its ball.  Raises ValueError for a
    table without a bound (an empty one, a Sierpinski, a 2-D Mandelbrot as an object): pass bounds to scene_mesh yourself then."""
    import numpy as np
    out = (C.c_float * 14)()
    check(lib().rm_debug_cull_bounds(tables.objects, tables.num_objects, C.byref(tables.globals_), out))
    v = np.array(list(out), dtype=np.float64)
    if v[0] == 0.0:
        raise ValueError("the object table has no bound (rm_debug_cull_bounds): pass bounds=(lo, hi)")
    if v[6] != 0.0:
        lo, hi = v[7:10], v[10:13]
    else:
        r = np.sqrt(v[4])
        lo, hi = v[1:4] - r, v[1:4] + r
    return (lo - margin).astype(np.float32), (hi + margin).astype(np.float32)


def write_ply(path, vertices, quads, colours=None):
    """rm_write_ply: the mesh of extract_mesh / scene_mesh as a binary little-endian PLY.  vertices (n, 4) float32 and quads (m, 4)
    int32, tensors or arrays; colours: (n, 3) uint8 or None."""
    return write_ply_ex(path, vertices, quads, colours)


def write_ply_ex(path, vertices, quads, colours=None, normals=None):
    """write_ply with vertex normals, the mesh of bake_mesh as it is: normals (n, 3) or (n, 4) float32 or None — with them the file
    goes through rm_write_ply_ex and carries nx, ny, nz behind z; without them it is write_ply's file, byte for byte."""
    import numpy as np

    def host(a, dtype, cols):
        a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.ndim != 2 or a.shape[1] not in cols:
            raise ValueError(f"expected an (n, {cols[0]}) array, got {a.shape}")
        return a
    v, q = host(vertices, np.float32, (4,)), host(quads, np.int32, (4,))
    c = None if colours is None else host(colours, np.uint8, (3,))
    if c is not None and c.shape[0] != v.shape[0]:
        raise ValueError("one colour per vertex")
    cp = C.c_void_p(c.ctypes.data) if c is not None else None
    if normals is None:
        check(lib().rm_write_ply(str(path).encode(), C.c_void_p(v.ctypes.data), v.shape[0], C.c_void_p(q.ctypes.data), q.shape[0], cp))
        return path
    n3 = host(normals, np.float32, (3, 4))
    if n3.shape[0] != v.shape[0]:
        raise ValueError("one normal per vertex")
    n4 = np.zeros((v.shape[0], 4), dtype=np.float32)
    n4[:, :n3.shape[1]] = n3
    check(lib().rm_write_ply_ex(str(path).encode(), C.c_void_p(v.ctypes.data), v.shape[0], C.c_void_p(q.ctypes.data), q.shape[0], cp,
                                C.c_void_p(n4.ctypes.data)))
    return path


def hemisphere_directions(num_dirs, num_sets=1):
    """rm_hemisphere_directions: the table LatticeField.ambient builds for an int `directions` → float32 (num_sets·num_dirs, 4)
    numpy array of (x, y, z, weight) rows in a point's frame, z along its normal: a cosine-weighted spiral of num_dirs unit
    directions (a power of two, at most abi.RM_MAX_AMBIENT_DIRS) with weight 1 / num_dirs, turned by another angle in each set."""
    import numpy as np
    table = np.zeros((max(int(num_sets), 0) * max(int(num_dirs), 0), 4), dtype=np.float32)
    check(lib().rm_hemisphere_directions(int(num_dirs), int(num_sets), C.c_void_p(table.ctypes.data)))
    return table


def sphere_directions(num_dirs, num_sets=1):
    """rm_sphere_directions: the table Renderer.light_probes builds for an int `directions` → float32 (num_sets·num_dirs, 16) numpy
    array of RmProbeDir rows (dir.xyz, 0, the nine basis values, 0, 0, 0): num_dirs spherical Fibonacci directions (a power of two,
    at most abi.RM_MAX_PROBE_DIRS), turned about z by another angle in each set, and per direction 4π / num_dirs times the nine real
    spherical harmonics of bands 0 to 2 there."""
    import numpy as np
    table = np.zeros((max(int(num_sets), 0) * max(int(num_dirs), 0), 16), dtype=np.float32)
    check(lib().rm_sphere_directions(int(num_dirs), int(num_sets), C.c_void_p(table.ctypes.data)))
    return table


def probe_depth_weights(table, sets=1, sharpness=50.0):
    """rm_probe_depth_weights: the texel weights Renderer.light_probes_depth builds for a direction table → float32
    (sets·directions, 64) numpy array: row k's share of each texel of the 8×8 octahedral depth map, max(0, cos)^sharpness around the
    texel's centre direction, normalised per texel over the rows of the set.  table: float32 (sets·directions, 16) rows of
    RmProbeDir (sphere_directions' or the caller's own; the basis is not read).  A texel that no lobe reaches goes to the nearest
    row whole; the definition is in include/raymarcher_amd.h."""
    import numpy as np
    table = _np_f32(table)
    sets = int(sets)
    if table.ndim != 2 or table.shape[1] != 16 or sets < 1 or table.shape[0] % sets:
        raise ValueError("table must be float32 (sets * directions, 16) rows of RmProbeDir")
    out = np.zeros((table.shape[0], abi.RM_PROBE_DEPTH_TEXELS), dtype=np.float32)
    check(lib().rm_probe_depth_weights(C.c_void_p(table.ctypes.data), table.shape[0] // sets, sets, float(sharpness), C.c_void_p(out.ctypes.data)))
    return out


def sh_irradiance(sh, normals):
    """The irradiance that SH9 radiance coefficients give a surface with unit normal n: the clamped-cosine convolution
    E(n) = Σ_j A_band(j)·sh_j·Y_j(n) with A = π, 2π/3, π/4 for bands 0, 1, 2 (Ramamoorthi & Hanrahan 2001).  sh: (..., 9, c) —
    light_probes' `sh`, whose fourth channel convolves like the others —, normals: (..., 3), broadcast against sh's leading
    dimensions → (..., c).  Torch tensors or NumPy arrays, in their own precision; plain array arithmetic, not bit-defined."""
    import math
    x, y, z = normals[..., 0], normals[..., 1], normals[..., 2]
    c1, c2 = math.sqrt(3.0 / (4.0 * math.pi)), math.sqrt(15.0 / (4.0 * math.pi))
    a0, a1, a2 = math.pi, 2.0 * math.pi / 3.0, math.pi / 4.0
    weights = (a0 * math.sqrt(1.0 / (4.0 * math.pi)) * (x * 0 + 1), a1 * c1 * y, a1 * c1 * z, a1 * c1 * x, a2 * c2 * (x * y), a2 * c2 * (y * z),
               a2 * math.sqrt(5.0 / (16.0 * math.pi)) * (3.0 * (z * z) - 1.0), a2 * c2 * (x * z),
               a2 * math.sqrt(15.0 / (16.0 * math.pi)) * (x * x - y * y))
    total = None
    for j, w in enumerate(weights):
        term = sh[..., j, :] * w[..., None]
        total = term if total is None else total + term
    return total


class LatticeField:
    """An RmField handle (Renderer.lattice_field, lattice_field_blocks, scene_field): one lattice queried again and again.  It keeps
    references to the tensors the handle borrows.  A context manager; close() is idempotent, and the handle is destroyed on garbage
    collection at the latest.  Synchronise the streams that still run its queries before closing it."""

    def __init__(self, renderer, handle, borrowed, box=None):
        """box: (origin, step, cells per axis) of the lattice, which ambient's defaults are taken from."""
        self._r, self._h, self._borrowed, self._box = renderer, handle, borrowed, box
        self._tables = {}  # ambient's tables on the device, per (dirs, sets)

    def close(self):
        h, self._h = self._h, None
        if h:
            lib().rm_field_destroy(h)
        self._borrowed = None
        self._tables = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self._h:
            raise ValueError("the LatticeField is closed")
        return self._h

    def sample(self, points):
        """rm_field_sample → sample_lattice's 4-tuple (gradient, value, cell, object_id), in every bit."""
        r, h = self._r, self._handle()
        t = r.torch
        pts = r._points(points, "points")
        n = pts.shape[0]
        out = t.empty((n, 8), dtype=t.float32, device=r.device)
        check(lib().rm_field_sample(h, C.c_void_p(pts.data_ptr()) if n else None, n, C.c_void_p(out.data_ptr()) if n else None, r._stream()))
        return out[:, 0:3], out[:, 3], out[:, 4:7].view(t.int32), out[:, 7].view(t.int32)

    def trace(self, rays, iso=0.001, max_steps=256, mode="closest", normals=True, out=None):
        """rm_field_trace → trace_lattice's 4-tuple (normal, t, position, object_id).  max_steps counts samples only: crossing
        unlisted blocks is free.  mode "occlusion", trace_rays' spelling: object_id = the occluder's id (−1: none), t = the penumbra
        factor; visibility is t where object_id == −1, else 0."""
        r, h = self._r, self._handle()
        t = r.torch
        if mode not in ("closest", "occlusion"):
            raise ValueError(f"mode = {mode!r}: 'closest' or 'occlusion'")
        rays = r._rays(rays)
        n = rays.shape[0]
        hits = r._out(out, (n, 8), t.float32)
        bits = abi.RM_TRACE_OCCLUSION if mode == "occlusion" else (abi.RM_TRACE_CLOSEST if normals else abi.RM_TRACE_NO_NORMAL)
        check(lib().rm_field_trace(h, C.c_void_p(rays.data_ptr()) if n else None, n, float(iso), int(max_steps), bits,
                                   C.c_void_p(hits.data_ptr()) if n else None, r._stream()))
        return hits[:, 0:3], hits[:, 3], hits[:, 4:7], hits[:, 7].view(t.int32)

    def ambient(self, points, normals=None, directions=16, sets=1, max_distance=None, bias=None, iso=0.001, max_steps=64, soft=True, out=None):
        """rm_field_ambient: hemisphere occlusion and the bent normal at points of the lattice, `directions` rays per point marched
        and summed in ONE launch, with no per-ray memory → (bent, visibility, normal, hits): float32 (n, 3), (n), (n, 3) and int32
        (n), views of ONE float32 (n, 8) device tensor of RmAmbient rows (`out`, if given).  points as sample takes them; normals:
        the same shapes, unit vectors, or None for the lattice's own normalised gradient.  directions: an int, a power of two up to
        abi.RM_MAX_AMBIENT_DIRS — hemisphere_directions(directions, sets), built once per (directions, sets) and kept on the handle
        — or a ready float32 (sets·dirs, 4) table of (x, y, z, weight) rows in the point's frame, z along the normal; point i uses
        set i mod sets.  soft: every ray contributes its penumbra factor (trace's "occlusion" march); otherwise 1 or 0.  visibility
        is the weighted sum over the rays, with the built table the cosine-weighted open fraction of the hemisphere; bent is the
        same sum of the directions, not normalised; hits counts the rays that hit, or is abi.RM_RAY_INVALID, abi.RM_FIELD_OUTSIDE or
        abi.RM_FIELD_UNLISTED beside zeros for a point that has no normal.  max_distance (None: the diagonal of the lattice's box)
        is every ray's tMax.  bias (None: twice the largest lattice step) moves the ray origins along the normal and must exceed
        iso: at p + bias·n the field is about bias, and a ray whose first sample lies below iso is a hit at once.  The definition,
        bit for bit, is in include/raymarcher_amd.h."""
        r, h = self._r, self._handle()
        t = r.torch
        pts = r._points(points, "points")
        n = pts.shape[0]
        nrm = None if normals is None else r._points(normals, "normals")
        if nrm is not None and nrm.shape[0] != n:
            raise ValueError("one normal per point")
        sets = int(sets)
        if isinstance(directions, int):
            dirs = int(directions)
            key = (dirs, sets)
            if key not in self._tables:
                self._tables[key] = t.from_numpy(hemisphere_directions(dirs, sets)).to(r.device)
            table = self._tables[key]
        else:
            table = directions if t.is_tensor(directions) else t.from_numpy(_np_f32(directions))
            if table.dim() != 2 or table.shape[1] != 4 or table.dtype != t.float32 or sets < 1 or table.shape[0] % sets != 0:
                raise ValueError("directions must be an int or a float32 table of shape (sets * dirs, 4)")
            table = table.to(r.device).contiguous()
            dirs = table.shape[0] // sets
        if (bias is None or max_distance is None) and self._box is None:
            raise ValueError("this LatticeField does not know its lattice: give bias and max_distance")
        if bias is None:
            bias = 2.0 * max(float(v) for v in self._box[1])
        if max_distance is None:
            max_distance = sum((float(v) * c) ** 2 for v, c in zip(self._box[1], self._box[2])) ** 0.5
        rec = r._out(out, (n, 8), t.float32)
        check(lib().rm_field_ambient(h, C.c_void_p(pts.data_ptr()) if n else None, C.c_void_p(nrm.data_ptr()) if nrm is not None and n else None, n,
                                     C.c_void_p(table.data_ptr()) if table.numel() else None, dirs, sets, float(bias), float(max_distance),
                                     float(iso), int(max_steps), abi.RM_AMBIENT_SOFT if soft else abi.RM_AMBIENT_HARD,
                                     C.c_void_p(rec.data_ptr()) if n else None, r._stream()))
        return rec[:, 0:3], rec[:, 3], rec[:, 4:7], rec[:, 7].view(t.int32)


def _np_f32(a):
    import numpy as np
    return np.ascontiguousarray(a, dtype=np.float32)


def _grid_dims(dims):
    nx, ny, nz = (int(d) for d in dims)
    if min(nx, ny, nz) < 2:
        raise ValueError("a light grid has at least 2 probes along every axis")
    return nx, ny, nz


def light_grid_positions(origin, step, dims):
    """The world positions of a light grid's probes → float32 (nx·ny·nz, 4) numpy array, w = 0, x fastest: probe (i, j, k) is row
    i + nx·(j + ny·k) at origin + (i, j, k)·step, each coordinate one float32 multiplication and one float32 addition — the formula
    of rm_light_grid_irradiance (include/raymarcher_amd.h), so probes baked at these positions are where the lookup thinks they are."""
    import numpy as np
    nx, ny, nz = _grid_dims(dims)
    o, s = np.asarray(origin, dtype=np.float32).reshape(3), np.asarray(step, dtype=np.float32).reshape(3)
    axes = [o[a] + np.arange(n, dtype=np.float32) * s[a] for a, n in enumerate((nx, ny, nz))]
    out = np.zeros((nz, ny, nx, 4), dtype=np.float32)
    out[..., 0], out[..., 1], out[..., 2] = axes[0][None, None, :], axes[1][None, :, None], axes[2][:, None, None]
    return out.reshape(nx * ny * nz, 4)


class LightGrid:
    """A grid of SH9 radiance probes and the box it spans (Renderer.light_grid bakes one; LightGrid(renderer, probes, origin, step,
    dims) wraps a caller's own records): `probes` is the float32 (nx·ny·nz, 40) tensor of RmLightProbe rows as light_probes stores
    them, probe (i, j, k) at row i + nx·(j + ny·k) and at origin + (i, j, k)·step (light_grid_positions).  A probe whose hits is
    negative (abi.RM_RAY_INVALID) is left out of every lookup.  A numpy array is uploaded, a tensor on the renderer's device is kept
    as it is.  `depth` is None, or — Renderer.light_grid_visible bakes them, set_depth attaches a caller's own — the probes' depth
    moments, with which every lookup weighs a probe by whether it sees the point."""

    def __init__(self, renderer, probes, origin, step, dims):
        import numpy as np
        t = renderer.torch
        self.dims = _grid_dims(dims)
        if not t.is_tensor(probes):
            probes = t.from_numpy(_np_f32(probes)).to(renderer.device)
        count = self.dims[0] * self.dims[1] * self.dims[2]
        if (tuple(probes.shape) != (count, 40) or probes.dtype != t.float32 or not probes.is_contiguous() or probes.device != renderer.device):
            raise ValueError(f"probes must be a contiguous float32 tensor of shape ({count}, 40) on {renderer.device}")
        self._r, self.probes, self.depth, self.normal_bias = renderer, probes, None, None
        self.origin, self.step = np.asarray(origin, dtype=np.float32).reshape(3).copy(), np.asarray(step, dtype=np.float32).reshape(3).copy()

    def set_depth(self, depth, normal_bias=None):
        """Attaches (None: removes) the probes' depth moments → self: float32 (nx·ny·nz, 64, 2), RmProbeDepth rows as
        Renderer.light_probes_depth stores them, probe order as `probes`; a numpy array is uploaded, a tensor on the renderer's
        device is kept as it is.  From then on irradiance, light_gbuffer and Renderer.render_indirect take the visible lookup.
        normal_bias: the default bias of those lookups, None = 0.25 × the smallest step."""
        t = self._r.torch
        if depth is not None:
            if not t.is_tensor(depth):
                depth = t.from_numpy(_np_f32(depth)).to(self._r.device)
            count = self.dims[0] * self.dims[1] * self.dims[2]
            if (tuple(depth.shape) != (count, 64, 2) or depth.dtype != t.float32 or not depth.is_contiguous() or depth.device != self._r.device):
                raise ValueError(f"depth must be a contiguous float32 tensor of shape ({count}, 64, 2) on {self._r.device}")
        self.depth, self.normal_bias = depth, normal_bias
        return self

    def irradiance(self, points, normals, facing=True, out=None):
        """rm_light_grid_irradiance: the grid's light at `points` on surfaces with `normals`, ONE launch → (e, weight, probes): float32
        (n, 4), float32 (n) and int32 (n), views of ONE float32 (n, 8) device tensor of RmGridLight rows (`out`, if given).  points,
        normals: (n, 3) or (n, 4) float32, numpy arrays, which are uploaded, or tensors, used in place; normals are used as given
        (unit vectors are meant).  e[:, 0:3] is the irradiance — the eight probes around the point blended trilinearly, invalid probes
        left out, each convolved with the normal's cosine lobe; times albedo / π it is the diffuse light a surface sends on — and
        1 − e[:, 3] / π the cosine-weighted sky visibility.  facing: DDGI's backface term, which takes weight from probes behind the
        surface.  weight: the sum of the eight weights; probes: how many corners took part, 0 (zeros in e) where none did,
        abi.RM_RAY_INVALID for a non-finite point or a non-finite or zero normal.  A point outside the box takes the border's light.
        A grid that has depth records takes irradiance_visible's lookup with its defaults; one without gives what it always gave.
        The definition, bit for bit, is in include/raymarcher_amd.h."""
        return self.irradiance_visible(points, normals, facing=facing, out=out)

    def irradiance_visible(self, points, normals, facing=True, out=None, visible=None, normal_bias=None):
        """irradiance with the choice of the lookup.  visible: True — rm_light_grid_irradiance_visible, which also weighs every probe
        by the Chebyshev visibility of the point q = p + normal_bias·n in the probe's depth map, so that light does not leak through
        walls (the grid must have depth records) —, False — rm_light_grid_irradiance —, None — whichever the grid has records for.
        normal_bias: None = the grid's normal_bias, and 0.25 × the smallest step where that is None too.  The definition, bit for
        bit, is in include/raymarcher_amd.h."""
        r = self._r
        t = r.torch
        pts, nrm = r._points(points, "points"), r._points(normals, "normals")
        n = pts.shape[0]
        if nrm.shape[0] != n:
            raise ValueError("one normal per point")
        visible = self.depth is not None if visible is None else bool(visible)
        if visible and self.depth is None:
            raise ValueError("visible=True needs a grid with depth records (Renderer.light_grid_visible, LightGrid.set_depth)")
        rec = r._out(out, (n, 8), t.float32)
        if visible:
            bias = self.normal_bias if normal_bias is None else normal_bias
            bias = 0.25 * float(self.step.min()) if bias is None else float(bias)
            check(lib().rm_light_grid_irradiance_visible(
                C.c_void_p(self.probes.data_ptr()), C.c_void_p(self.depth.data_ptr()), (C.c_int * 3)(*self.dims), _vec3(self.origin, "origin"),
                _vec3(self.step, "step"), C.c_void_p(pts.data_ptr()) if n else None, C.c_void_p(nrm.data_ptr()) if n else None, n,
                abi.RM_LIGHT_GRID_FACING if facing else 0, bias, C.c_void_p(rec.data_ptr()) if n else None, r._stream()))
            return rec[:, 0:4], rec[:, 4], rec[:, 5].view(t.int32)
        check(lib().rm_light_grid_irradiance(C.c_void_p(self.probes.data_ptr()), (C.c_int * 3)(*self.dims), _vec3(self.origin, "origin"),
                                             _vec3(self.step, "step"), C.c_void_p(pts.data_ptr()) if n else None,
                                             C.c_void_p(nrm.data_ptr()) if n else None, n, abi.RM_LIGHT_GRID_FACING if facing else 0,
                                             C.c_void_p(rec.data_ptr()) if n else None, r._stream()))
        return rec[:, 0:4], rec[:, 4], rec[:, 5].view(t.int32)

    def ref(self, strength=1.0, facing=True, visible=None, normal_bias=None):
        """The grid as rm_shade_rays_indirect and rm_light_probes_indirect take it → abi.RmLightGridRef (it holds device pointers
        of this grid's tensors: keep the grid alive while a call that was given it runs).  facing, visible and normal_bias are
        irradiance_visible's: visible=None takes the depth records where the grid has them."""
        visible = self.depth is not None if visible is None else bool(visible)
        if visible and self.depth is None:
            raise ValueError("visible=True needs a grid with depth records (Renderer.light_grid_visible, LightGrid.set_depth)")
        bias = self.normal_bias if normal_bias is None else normal_bias
        bias = 0.25 * float(self.step.min()) if bias is None else float(bias)
        return abi.RmLightGridRef(self.probes.data_ptr(), self.depth.data_ptr() if visible else None, (C.c_int32 * 3)(*self.dims),
                                  (C.c_float * 3)(*self.origin), (C.c_float * 3)(*self.step), float(strength),
                                  abi.RM_LIGHT_GRID_FACING if facing else 0, bias)

    def light_gbuffer(self, normal_depth, position, facing=True):
        """irradiance at the primary hits of render_gbuffer(position=True): normal_depth and position, float32 (N, H, W, 4) as it
        returns them, used in place → float32 (N, H, W, 4), e per pixel (a view of the (N·H·W, 8) result).  A miss has a zero normal,
        which makes it an invalid point: zeros.  Follows the grid as irradiance does."""
        return self.light_gbuffer_visible(normal_depth, position, facing=facing)

    def light_gbuffer_visible(self, normal_depth, position, facing=True, visible=None, normal_bias=None):
        """light_gbuffer with irradiance_visible's `visible` and `normal_bias`."""
        t = self._r.torch
        if (normal_depth.dim() != 4 or normal_depth.shape[3] != 4 or tuple(position.shape) != tuple(normal_depth.shape)
                or normal_depth.dtype != t.float32 or position.dtype != t.float32):
            raise ValueError("normal_depth and position must be float32 tensors of the same shape (N, H, W, 4)")
        N, H, W, _ = normal_depth.shape
        e, _, _ = self.irradiance_visible(position.reshape(-1, 4), normal_depth.reshape(-1, 4), facing=facing, visible=visible,
                                          normal_bias=normal_bias)
        return e.view(N, H, W, 4)


class Renderer:
    """Launches the HIP raymarch on one GPU; outputs are torch tensors on that device."""

    def __init__(self, device=0):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("raymarcher_amd.Renderer needs a HIP device; there is no CPU fallback")
        self.torch = torch
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        check(lib().rm_set_device(device))
        # _upload's cache: id(host array) → (the array, its device copy).  Threads may share a Renderer (each on a stream of its own),
        # so the dict exists before any of them runs and every look-up and insertion holds the lock: an entry, once made, keeps the
        # device tensor that an enqueued launch reads alive.
        self._tex_cache = {}
        self._tex_lock = threading.Lock()
        self._probe_tables = {}  # light_probes' tables on the device, per (directions, sets); under the same lock
        self._depth_weights = {}  # light_probes_depth's weights of those tables, per (directions, sets, sharpness); under the same lock

    def _out(self, a, shape, dtype, name="out"):
        """A fresh tensor of `shape` and `dtype` on this device, or the caller's `a` once it is checked to be exactly that (the
        kernels write every element of it and nothing past it)."""
        t = self.torch
        if a is None:
            return t.empty(shape, dtype=dtype, device=self.device)
        if tuple(a.shape) != tuple(shape) or a.dtype != dtype or not a.is_contiguous() or a.device != self.device:
            raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {self.device}")
        return a

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _upload(self, a):
        """Host uint8 array → device tensor, cached per array object."""
        key = id(a)
        with self._tex_lock:
            if key not in self._tex_cache:
                self._tex_cache[key] = (a, self.torch.from_numpy(a).contiguous().to(self.device))
            return self._tex_cache[key][1]

    def _resources(self, tables):
        """RmResources with device pointers for everything `tables` carries; returns (struct, keep-alive list)."""
        res = abi.RmResources()
        keep = []

        def fill(slot, a):
            dev = self._upload(a)
            keep.append(dev)
            slot.pixels = dev.data_ptr()
            slot.height, slot.width = a.shape[0], a.shape[1]

        host = tables.textures or []
        if host:
            arr = (abi.RmTexture * len(host))()
            for i, a in enumerate(host):
                fill(arr[i], a)
            keep.append(arr)
            res.textures = arr
            res.numTextures = len(host)
        if tables.noise is not None:
            fill(res.noise, tables.noise)
        if tables.skybox:
            if len(tables.skybox) != 6:
                raise ValueError("skybox needs six faces (+X,-X,+Y,-Y,+Z,-Z)")
            for f in range(6):
                fill(res.skybox[f], tables.skybox[f])
        for name in ("ltc1", "ltc2"):
            a = getattr(tables, name)
            if a is not None:
                if a.shape != (abi.RM_LTC_SIZE, abi.RM_LTC_SIZE, 4) or str(a.dtype) != "uint8":
                    raise ValueError(f"{name} must be uint8 (64, 64, 4); see ltc_quantise")
                dev = self._upload(a)
                keep.append(dev)
                setattr(res, name, dev.data_ptr())
        return res, keep

    def render(self, tables, settings, W, H, row_begin=0, row_end=None, bright=False, out=None, out_bright=None):
        """rm_render: rows [row_begin,row_end) → float32 tensor (rows, W, 4), row 0 = bottom.  out / out_bright: the caller's
        buffers for the frame and (implying bright=True) its BrightColor."""
        t = self.torch
        row_end = H if row_end is None else row_end
        shape = (max(row_end - row_begin, 0), W, 4)
        out = self._out(out, shape, t.float32)
        bright = bright or out_bright is not None
        br = self._out(out_bright, shape, t.float32, "out_bright") if bright else None
        res, _keep = self._resources(tables)
        check(lib().rm_render_res(*tables.args(settings), C.byref(res), W, H, row_begin, row_end, C.c_void_p(out.data_ptr()),
                                  C.c_void_p(br.data_ptr()) if bright else None, self._stream()))
        return (out, br) if bright else out

    def _render_frames(self, entry, tables, settings, W, H, cameras, globals_, bright, out, out_bright, mid=(), extra=None,
                       sub_frames=None):
        """What render_batch, render_supersampled, render_adaptive and render_accumulated share: the batch arrays, the checked or
        fresh (N, H, W, 4) outputs, the resources, the call of lib().<entry> and the return value.  mid: the entry point's arguments
        between H and d_rgba.  extra(n): its optional outputs after d_bright, tensors or None, which join the returned tuple.
        sub_frames (render_accumulated): that many cameras per output frame, passed behind numFrames."""
        cams, globs = batch_arrays(cameras, tables.globals_ if globals_ is None else globals_)
        n = len(cameras) if sub_frames is None else len(cameras) // sub_frames
        counts = (n,) if sub_frames is None else (n, sub_frames)
        shape = (n, H, W, 4)
        t = self.torch
        out = self._out(out, shape, t.float32)
        bright = bright or out_bright is not None
        br = self._out(out_bright, shape, t.float32, "out_bright") if bright else None
        more = extra(n) if extra else ()
        res, _keep = self._resources(tables)
        ptrs = [C.c_void_p(a.data_ptr()) if a is not None else None for a in (out, br, *more)]
        check(getattr(lib(), entry)(cams, globs, len(globs), *counts, tables.objects, tables.num_objects, tables.lights, tables.num_lights,
                                    C.byref(settings), C.byref(res), W, H, *mid, *ptrs, self._stream()))
        rest = [x for x in (br, *more) if x is not None]
        return (out, *rest) if rest else out

    def render_batch(self, tables, settings, W, H, cameras, globals_=None, bright=False, out=None, out_bright=None):
        """rm_render_batch: N whole frames of the scene in `tables`, frame i seen through cameras[i] (RmCamera, as build_camera
        returns them) → float32 tensor (N, H, W, 4), row 0 = bottom.  globals_: None (tables.globals_ for every frame), one
        RmGlobals for every frame, or a sequence of N of them.  out / out_bright: the caller's buffers (out_bright implies
        bright=True)."""
        return self._render_frames("rm_render_batch", tables, settings, W, H, cameras, globals_, bright, out, out_bright)

    def render_supersampled(self, tables, settings, W, H, cameras, ss, globals_=None, bright=False, out=None, out_bright=None):
        """rm_render_supersampled: render_batch with ss × ss samples per pixel (ss = 1, 2 or 4), resolved inside the kernel by the
        fixed reduction tree of include/raymarcher_amd.h → float32 tensor (N, H, W, 4), row 0 = bottom.  Every other argument as
        render_batch's; ss = 1 is render_batch."""
        if ss not in (1, 2, 4):
            raise ValueError(f"ss = {ss!r}: the samples per pixel along each axis are 1, 2 or 4")
        return self._render_frames("rm_render_supersampled", tables, settings, W, H, cameras, globals_, bright, out, out_bright, mid=(ss,))

    def render_adaptive(self, tables, settings, W, H, cameras, ss, threshold, globals_=None, bright=False, out=None, out_bright=None,
                        mask=False, counts=False):
        """rm_render_adaptive: render_batch's frames with the pixels that differ from a 4-neighbour by more than `threshold` in r, g
        or b replaced by render_supersampled's (the definition is in include/raymarcher_amd.h) → float32 tensor (N, H, W, 4), row 0
        = bottom; with bright, mask (uint8 (N, H, W), 1 = refined) or counts (int32 (N,), refined pixels per frame, left on the
        device) a tuple (frames[, bright][, mask][, counts]).  mask / counts: True, or the caller's buffer of that shape and
        type.  Every other argument as render_supersampled's."""
        if ss not in (1, 2, 4):
            raise ValueError(f"ss = {ss!r}: the samples per pixel along each axis are 1, 2 or 4")
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("threshold is NaN")

        def extra(n):
            t = self.torch
            want_mask, want_counts = mask is not False and mask is not None, counts is not False and counts is not None
            m = self._out(None if mask is True else mask, (n, H, W), t.uint8, "mask") if want_mask else None
            cnt = self._out(None if counts is True else counts, (n,), t.int32, "counts") if want_counts else None
            return m, cnt

        return self._render_frames("rm_render_adaptive", tables, settings, W, H, cameras, globals_, bright, out, out_bright,
                                   mid=(ss, threshold), extra=extra)

    def render_accumulated(self, tables, settings, W, H, cameras, sub_frames, globals_=None, bright=False, out=None, out_bright=None):
        """rm_render_accumulated: N = len(cameras) / sub_frames frames, frame f the mean of render_batch's frames for
        cameras[f·sub_frames : (f + 1)·sub_frames] — summed in that order inside the kernel, then · 1 / sub_frames; the definition is
        in include/raymarcher_amd.h — → float32 tensor (N, H, W, 4), row 0 = bottom.  Depth of field: lens_cameras(...); motion
        blur: globals_=shutter_globals(...).  globals_: None (tables.globals_ for every sub-frame), one RmGlobals, or one per
        camera.  Every other argument as render_batch's; sub_frames = 1 is render_batch."""
        if not isinstance(sub_frames, int) or isinstance(sub_frames, bool) or not 1 <= sub_frames <= abi.RM_MAX_SUBFRAMES:
            raise ValueError(f"sub_frames = {sub_frames!r}: an integer from 1 to RM_MAX_SUBFRAMES = {abi.RM_MAX_SUBFRAMES}")
        if len(cameras) % sub_frames:
            raise ValueError(f"{len(cameras)} cameras are not a whole number of frames of {sub_frames} sub-frames")
        return self._render_frames("rm_render_accumulated", tables, settings, W, H, cameras, globals_, bright, out, out_bright,
                                   sub_frames=sub_frames)

    def render_animated(self, tables, settings, W, H, cameras, sub_frames=1, objects=None, lights=None, globals_=None, bright=False,
                        out=None, out_bright=None):
        """rm_render_animated: render_accumulated where every camera (block) may have an object table and a light table of its own
        → float32 tensor (len(cameras) / sub_frames, H, W, 4), row 0 = bottom.  objects / lights: None (tables.objects /
        tables.lights for every block) or the per-block tables, shape (blocks, tables.num_objects) / (blocks, tables.num_lights) of
        RmObject / RmLight — nested sequences or one flat ctypes array, e.g. translated_objects(...).  Every other argument as
        render_accumulated's; the definition is in include/raymarcher_amd.h."""
        if not isinstance(sub_frames, int) or isinstance(sub_frames, bool) or not 1 <= sub_frames <= abi.RM_MAX_SUBFRAMES:
            raise ValueError(f"sub_frames = {sub_frames!r}: an integer from 1 to RM_MAX_SUBFRAMES = {abi.RM_MAX_SUBFRAMES}")
        if len(cameras) % sub_frames:
            raise ValueError(f"{len(cameras)} cameras are not a whole number of frames of {sub_frames} sub-frames")
        cams, globs = batch_arrays(cameras, tables.globals_ if globals_ is None else globals_)
        blocks = len(cameras)
        objs, n_obj_tables = _stacked_tables(objects, "objects", abi.RmObject, tables.num_objects, blocks)
        lts, n_light_tables = _stacked_tables(lights, "lights", abi.RmLight, tables.num_lights, blocks)
        n = blocks // sub_frames
        t = self.torch
        out = self._out(out, (n, H, W, 4), t.float32)
        bright = bright or out_bright is not None
        br = self._out(out_bright, (n, H, W, 4), t.float32, "out_bright") if bright else None
        res, _keep = self._resources(tables)
        check(lib().rm_render_animated(cams, globs, len(globs), tables.objects if objs is None else objs, tables.num_objects, n_obj_tables,
                                       tables.lights if lts is None else lts, tables.num_lights, n_light_tables, n, sub_frames,
                                       C.byref(settings), C.byref(res), W, H, C.c_void_p(out.data_ptr()),
                                       C.c_void_p(br.data_ptr()) if bright else None, self._stream()))
        return (out, br) if bright else out

    def render_gbuffer(self, tables, settings, W, H, cameras=None, globals_=None, position=False, out_normal_depth=None,
                       out_object_id=None, out_position=None):
        """rm_render_gbuffer: what the primary ray of every pixel hit, N frames in one launch → (normal_depth, object_id[, position]):
        float32 (N, H, W, 4) = (n.x, n.y, n.z, depth along the ray), int32 (N, H, W) = the object's index in tables.objects (−1: a
        miss, with depth = the camera's initialFar and a zero normal) and, with position, float32 (N, H, W, 4) = (p.x, p.y, p.z,
        1 for a hit / 0).  Row 0 = bottom.  cameras: None (the scene's own camera, N = 1) or a sequence of RmCamera; globals_ as
        render_batch's.  Lights, textures and the shading settings play no part; the definition is in include/raymarcher_amd.h.
        out_*: the caller's buffers (out_position implies position=True)."""
        t = self.torch
        cams, globs = batch_arrays([tables.camera] if cameras is None else cameras, tables.globals_ if globals_ is None else globals_)
        n = 1 if cameras is None else len(cameras)
        nd = self._out(out_normal_depth, (n, H, W, 4), t.float32, "out_normal_depth")
        ids = self._out(out_object_id, (n, H, W), t.int32, "out_object_id")
        position = position or out_position is not None
        pos = self._out(out_position, (n, H, W, 4), t.float32, "out_position") if position else None
        check(lib().rm_render_gbuffer(cams, globs, len(globs), n, tables.objects, tables.num_objects, C.byref(settings), W, H,
                                      C.c_void_p(nd.data_ptr()), C.c_void_p(ids.data_ptr()),
                                      C.c_void_p(pos.data_ptr()) if position else None, self._stream()))
        return (nd, ids, pos) if position else (nd, ids)

    def trace_rays(self, tables, settings, rays, mode="closest", normals=True, out=None):
        """rm_trace_rays: what arbitrary rays hit, one lane per ray in one launch → (normal, t, position, object_id): float32 (n, 3),
        float32 (n), float32 (n, 3) and int32 (n), views of ONE float32 (n, 8) device tensor of RmRayHit rows (`out`, if given).
        rays: float32 (n, 8) rows of RmRay (origin.xyz, tMax, dir.xyz, unused) — a numpy array, which is uploaded, or a tensor on
        this device; dir is used as given, so t is in units of |dir|.  mode "closest": object_id = the object's index in
        tables.objects (−1: a miss, with t = tMax and zeros; abi.RM_RAY_INVALID: a non-finite or zero ray), t, the surface point
        and its normal; normals=False leaves the point and the normal out (zeros).  mode "occlusion": the renderer's shadow march:
        object_id = the occluder (−1: none), t = the penumbra factor; visibility is t where object_id == −1, else 0.  Lights,
        textures, the camera and the shading settings play no part; the definition is in include/raymarcher_amd.h."""
        t = self.torch
        if mode not in ("closest", "occlusion"):
            raise ValueError(f"mode = {mode!r}: 'closest' or 'occlusion'")
        rays = self._rays(rays)
        n = rays.shape[0]
        hits = self._out(out, (n, 8), t.float32)
        bits = abi.RM_TRACE_OCCLUSION if mode == "occlusion" else (abi.RM_TRACE_CLOSEST if normals else abi.RM_TRACE_NO_NORMAL)
        check(lib().rm_trace_rays(C.c_void_p(rays.data_ptr()), n, tables.objects, tables.num_objects, C.byref(tables.globals_),
                                  C.byref(settings), bits, C.c_void_p(hits.data_ptr()), self._stream()))
        return hits[:, 0:3], hits[:, 3], hits[:, 4:7], hits[:, 7].view(t.int32)

    def _rays(self, rays):
        """`rays` as trace_rays and shade_rays take them: a numpy array is uploaded, a tensor on this device is used in place."""
        t = self.torch
        if not t.is_tensor(rays):
            import numpy as np
            rays = t.from_numpy(np.ascontiguousarray(rays, dtype=np.float32)).to(self.device)
        if rays.dim() != 2 or rays.shape[1] != 8 or rays.dtype != t.float32 or not rays.is_contiguous() or rays.device != self.device:
            raise ValueError(f"rays must be a contiguous float32 tensor of shape (n, 8) on {self.device}")
        return rays

    def shade_rays(self, tables, settings, rays, far=None, bright=False, out=None, out_bright=None):
        """rm_shade_rays: the renderer's full colour for arbitrary rays, one lane per ray in one launch → float32 (n, 4), or the pair
        (colour, bright) with bright=True or out_bright.  rays: float32 (n, 8) rows of RmRay (origin.xyz, unread, dir.xyz, unread) —
        a numpy array, which is uploaded, or a tensor on this device; dir is used as given and the shading assumes it unit.  far:
        the one march limit of the call, None = tables.camera.initialFar.  The colour of a ray is what render() has for a pixel
        with that primary ray: lights, materials, textures, sky box, reflection and refraction as `settings` say; a non-finite or
        zero ray gives (0, 0, 0, 0), alpha 0.  Terrain, clouds and sea are refused.  The definition is in
        include/raymarcher_amd.h."""
        t = self.torch
        rays = self._rays(rays)
        n = rays.shape[0]
        out = self._out(out, (n, 4), t.float32)
        bright = bright or out_bright is not None
        br = self._out(out_bright, (n, 4), t.float32, "out_bright") if bright else None
        res, _keep = self._resources(tables)
        check(lib().rm_shade_rays(C.c_void_p(rays.data_ptr()), n, tables.camera.initialFar if far is None else far, tables.objects,
                                  tables.num_objects, tables.lights, tables.num_lights, C.byref(tables.globals_), C.byref(settings),
                                  C.byref(res), C.c_void_p(out.data_ptr()), C.c_void_p(br.data_ptr()) if bright else None,
                                  self._stream()))
        return (out, br) if bright else out

    def light_probes(self, tables, settings, positions, directions=256, sets=1, far=None, table=None, out=None):
        """rm_light_probes: SH9 radiance probes at `positions`, `directions` rays each shaded as shade_rays shades them and summed per
        probe in ONE launch → (sh, hits): float32 (n, 9, 4) and int32 (n), views of ONE float32 (n, 40) device tensor of RmLightProbe
        rows (`out`, if given).  positions: (n, 3) or (n, 4) float32, a numpy array, which is uploaded, or a tensor.  The table is
        sphere_directions(directions, sets) — directions a power of two, at most abi.RM_MAX_PROBE_DIRS; probe i uses set i mod sets —
        built once per (directions, sets) and kept on the renderer, or the caller's `table`: float32 (sets·directions, 16) rows of
        RmProbeDir, numpy or a tensor on this device, any basis values (an ambient cube, fewer bands, importance weights).  far: the
        one march limit of the call, None = tables.camera.initialFar.  sh[:, j, 0:3] are the radiance coefficients with
        sphere_directions' table (sh_irradiance turns them into irradiance), sh[:, j, 3] the same projection of "the ray hit
        something"; hits: the rays that hit, abi.RM_RAY_INVALID for a probe with a non-finite position (zeros in sh).  Terrain,
        clouds and sea are refused.  The definition is in include/raymarcher_amd.h."""
        t = self.torch
        dirs, sets = int(directions), int(sets)
        pts = self._points(positions, "positions")
        n = pts.shape[0]
        table = self._probe_table(dirs, sets, table)
        rec = self._out(out, (n, 40), t.float32)
        res, _keep = self._resources(tables)
        check(lib().rm_light_probes(C.c_void_p(pts.data_ptr()) if n else None, n, C.c_void_p(table.data_ptr()), dirs, sets,
                                    tables.camera.initialFar if far is None else far, tables.objects, tables.num_objects, tables.lights,
                                    tables.num_lights, C.byref(tables.globals_), C.byref(settings), C.byref(res),
                                    C.c_void_p(rec.data_ptr()) if n else None, self._stream()))
        return rec[:, 0:36].view(n, 9, 4), rec[:, 36].view(t.int32)

    def _probe_table(self, dirs, sets, table):
        """light_probes' table on this device: sphere_directions(dirs, sets), built once per (dirs, sets) and kept, or the caller's
        `table` once it is checked."""
        t = self.torch
        if table is None:
            key = (dirs, sets)
            with self._tex_lock:
                if key not in self._probe_tables:
                    self._probe_tables[key] = t.from_numpy(sphere_directions(dirs, sets)).to(self.device)
                return self._probe_tables[key]
        if not t.is_tensor(table):
            table = t.from_numpy(_np_f32(table)).to(self.device)
        if (table.dim() != 2 or tuple(table.shape) != (sets * dirs, 16) or table.dtype != t.float32 or not table.is_contiguous()
                or table.device != self.device):
            raise ValueError(f"table must be a contiguous float32 tensor of shape (sets * directions, 16) on {self.device}")
        return table

    def light_probes_depth(self, tables, settings, positions, directions=256, sets=1, max_distance=None, table=None, weights=None,
                           sharpness=50.0, out=None):
        """rm_light_probes_depth: the depth moments of probes at `positions`, `directions` rays each marched as trace_rays marches
        them and summed per probe and texel in ONE launch → float32 (n, 64, 2) device tensor of RmProbeDepth rows (`out`, if
        given): per texel of an 8×8 octahedral map the weighted mean of the distance to the scene and of its square, which
        LightGrid.irradiance turns into a visibility term.  positions, directions, sets, table: as light_probes takes them — one
        table serves both bakes.  max_distance: where a ray that hits nothing is taken to end, None = tables.camera.initialFar; keep
        it near the probe spacing, since a mean over a lobe that mixes a wall with a far miss says little.  weights: None =
        probe_depth_weights(table, sets, sharpness) — built once per (directions, sets, sharpness) and kept on the renderer for the
        renderer's own tables; for a caller's `table` EVERY call copies the table to the host (which waits for the device), builds
        the weights there and uploads them, so build them once yourself and pass them — or float32 (sets·directions, 64), numpy or
        a tensor on this device.  A probe with a non-finite position stores zeros.  Terrain, clouds
        and sea are refused.  The definition is in include/raymarcher_amd.h."""
        t = self.torch
        dirs, sets = int(directions), int(sets)
        pts = self._points(positions, "positions")
        n = pts.shape[0]
        own_table = table is None
        table = self._probe_table(dirs, sets, table)
        if weights is None:
            key = (dirs, sets, float(sharpness))
            with self._tex_lock:
                weights = self._depth_weights.get(key) if own_table else None
            if weights is None:
                weights = t.from_numpy(probe_depth_weights(table.cpu().numpy(), sets, sharpness)).to(self.device)
                if own_table:
                    with self._tex_lock:
                        weights = self._depth_weights.setdefault(key, weights)
        else:
            if not t.is_tensor(weights):
                weights = t.from_numpy(_np_f32(weights)).to(self.device)
            if (tuple(weights.shape) != (sets * dirs, 64) or weights.dtype != t.float32 or not weights.is_contiguous()
                    or weights.device != self.device):
                raise ValueError(f"weights must be a contiguous float32 tensor of shape (sets * directions, 64) on {self.device}")
        rec = self._out(out, (n, 64, 2), t.float32)
        check(lib().rm_light_probes_depth(C.c_void_p(pts.data_ptr()) if n else None, n, C.c_void_p(table.data_ptr()),
                                          C.c_void_p(weights.data_ptr()), dirs, sets,
                                          tables.camera.initialFar if max_distance is None else max_distance, tables.objects,
                                          tables.num_objects, C.byref(tables.globals_), C.byref(settings),
                                          C.c_void_p(rec.data_ptr()) if n else None, self._stream()))
        return rec

    def light_grid(self, tables, settings, dims, bounds=None, directions=256, sets=1, far=None, mask_inside=0.0):
        """A LightGrid of dims = (nx, ny, nz) probes over `bounds` — (lo, hi), or None for mesh_bounds(tables) —, the first probe at
        lo and the last at hi: ONE light_probes call at light_grid_positions(origin, step, dims) with `directions`, `sets` and `far` as
        light_probes takes them.  mask_inside (None: no masking): one sdf_grid call on the same origin, step and dims, and every probe
        whose scene distance is below it gets hits = abi.RM_RAY_INVALID, so that LightGrid.irradiance leaves it out — 0.0 masks the
        probes inside geometry, whose rays see the inside of a surface."""
        return self._light_grid(tables, settings, dims, bounds, directions, sets, far, mask_inside, False)

    def light_grid_visible(self, tables, settings, dims, bounds=None, directions=256, sets=1, far=None, mask_inside=0.0, visibility=True,
                           sharpness=50.0):
        """light_grid, and with visibility ONE light_probes_depth call more at the same positions with the same table, the weights
        of probe_depth_weights(table, sets, sharpness) and max_distance = 1.5 × the length of `step`: the grid then carries depth
        records and its lookups weigh every probe by whether it sees the point, so that a lit room does not bleed through a wall
        into the dark room next to it."""
        return self._light_grid(tables, settings, dims, bounds, directions, sets, far, mask_inside, bool(visibility), sharpness)

    def _light_grid(self, tables, settings, dims, bounds, directions, sets, far, mask_inside, visibility, sharpness=50.0):
        import numpy as np
        t = self.torch
        nx, ny, nz = _grid_dims(dims)
        lo, hi = mesh_bounds(tables) if bounds is None else bounds
        lo, hi = np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(hi, dtype=np.float64).reshape(3)
        if not np.isfinite(hi - lo).all() or not (hi > lo).all():
            raise ValueError("bounds must be (lo, hi) with three finite components each and lo < hi")
        origin, step = lo.astype(np.float32), ((hi - lo) / (np.array([nx, ny, nz]) - 1)).astype(np.float32)
        rec = t.empty((nx * ny * nz, 40), dtype=t.float32, device=self.device)
        positions = self._points(light_grid_positions(origin, step, (nx, ny, nz)), "positions")
        _, hits = self.light_probes(tables, settings, positions, directions=directions, sets=sets, far=far, out=rec)
        if mask_inside is not None:
            dist = self.sdf_grid(tables, settings, origin, step, (nx, ny, nz))
            hits[dist.reshape(-1) < float(mask_inside)] = abi.RM_RAY_INVALID
        grid = LightGrid(self, rec, origin, step, (nx, ny, nz))
        if visibility:
            grid.set_depth(self.light_probes_depth(tables, settings, positions, directions=directions, sets=sets, sharpness=sharpness,
                                                   max_distance=1.5 * float(np.linalg.norm(step.astype(np.float64)))))
        return grid

    def render_indirect(self, tables, settings, W, H, grid, cameras=None, strength=1.0):
        """render_batch's frames plus one bounce of diffuse light from a LightGrid → float32 (N, H, W, 4): on every pixel whose
        primary ray hits an object, strength · kd · cDiffuse[object_id] · e.rgb / π is added to the colour, e = grid.light_gbuffer
        of one render_gbuffer(position=True) through the same cameras (None: the scene's own, N = 1) — with the visibility term where
        the grid has depth records (light_grid_visible), without it where not.  Plain torch arithmetic around
        the three launches, NOT bit-defined.  The albedo is the object's cDiffuse alone: textures and the fractals' trap colours are
        not part of it, and reflections and refractions get no indirect light."""
        import math
        t = self.torch
        cams = [tables.camera] if cameras is None else cameras
        frames = self.render_batch(tables, settings, W, H, cams)
        if tables.num_objects == 0:
            return frames
        nd, ids, pos = self.render_gbuffer(tables, settings, W, H, cams, position=True)
        e = grid.light_gbuffer(nd, pos)
        albedo = t.tensor([list(tables.objects[i].cDiffuse) for i in range(tables.num_objects)], dtype=t.float32, device=self.device)
        hit = ids >= 0
        bounce = albedo[ids.clamp(min=0).long()] * e[..., 0:3] * (float(strength) * float(tables.globals_.kd) / math.pi)
        frames[..., 0:3] += t.where(hit[..., None], bounce, t.zeros_like(bounce))
        return frames

    def shade_rays_indirect(self, tables, settings, rays, grid, far=None, strength=1.0, facing=True, visible=None, normal_bias=None,
                            out=None):
        """rm_shade_rays_indirect: shade_rays' colour with the diffuse light of `grid` (a LightGrid) added at every ray's primary hit,
        one lane per ray in ONE launch → float32 (n, 4).  rays and far: as shade_rays takes them.  At a hit the kernel looks the
        grid up at the hit point and the bumped normal — LightGrid.irradiance_visible's lookup with `facing`, `visible` and
        `normal_bias` —, clamps the irradiance at zero and adds strength · dif · e / π, dif the hit's diffuse colour WITH its
        texture, times the trap palette on the Mandelbulb and the Menger sponge.  Misses, emissive hits, invalid rays and hits that
        no probe reaches keep shade_rays' words; reflection and refraction bounces get no indirect light; there is no bright
        output.  Terrain, clouds and sea are refused.  The definition, bit for bit, is in include/raymarcher_amd.h."""
        t = self.torch
        rays = self._rays(rays)
        n = rays.shape[0]
        out = self._out(out, (n, 4), t.float32)
        res, _keep = self._resources(tables)
        ref = grid.ref(strength, facing, visible, normal_bias)
        check(lib().rm_shade_rays_indirect(C.c_void_p(rays.data_ptr()), n, tables.camera.initialFar if far is None else far, tables.objects,
                                           tables.num_objects, tables.lights, tables.num_lights, C.byref(tables.globals_),
                                           C.byref(settings), C.byref(res), C.byref(ref), C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def light_probes_indirect(self, tables, settings, positions, grid, directions=256, sets=1, far=None, table=None, strength=1.0,
                              facing=True, visible=None, normal_bias=None, out=None):
        """rm_light_probes_indirect: light_probes with every ray shaded as shade_rays_indirect shades it — the probes of the next
        bounce, from the grid of the bounce before, in ONE launch → (sh, hits) as light_probes.  positions, directions, sets, far,
        table: light_probes'; grid, strength, facing, visible, normal_bias: shade_rays_indirect's.  `out` must not be the grid's own
        records: the call is refused, ping-pong two buffers (light_grid_bounces does).  The definition is in
        include/raymarcher_amd.h."""
        t = self.torch
        dirs, sets = int(directions), int(sets)
        pts = self._points(positions, "positions")
        n = pts.shape[0]
        table = self._probe_table(dirs, sets, table)
        rec = self._out(out, (n, 40), t.float32)
        res, _keep = self._resources(tables)
        ref = grid.ref(strength, facing, visible, normal_bias)
        check(lib().rm_light_probes_indirect(C.c_void_p(pts.data_ptr()) if n else None, n, C.c_void_p(table.data_ptr()), dirs, sets,
                                             tables.camera.initialFar if far is None else far, tables.objects, tables.num_objects,
                                             tables.lights, tables.num_lights, C.byref(tables.globals_), C.byref(settings), C.byref(res),
                                             C.byref(ref), C.c_void_p(rec.data_ptr()) if n else None, self._stream()))
        return rec[:, 0:36].view(n, 9, 4), rec[:, 36].view(t.int32)

    def light_grid_bounces(self, tables, settings, dims, bounces=2, bounds=None, directions=256, sets=1, far=None, mask_inside=0.0,
                           visibility=True, strength=1.0):
        """A LightGrid that holds `bounces` further bounces of diffuse light: one light_grid / light_grid_visible bake (direct
        light at the probe rays' hits), then `bounces` calls of light_probes_indirect at the same positions, each reading the
        grid of the call before it and writing the other of two record buffers.  The depth records and the inside mask are made
        once, by the first bake, and carried along.  → the last LightGrid; bounces=0 is light_grid_visible's."""
        t = self.torch
        grid = self._light_grid(tables, settings, dims, bounds, directions, sets, far, mask_inside, bool(visibility))
        if int(bounces) <= 0:
            return grid
        positions = self._points(light_grid_positions(grid.origin, grid.step, grid.dims), "positions")
        masked = grid.probes[:, 36].view(t.int32) < 0
        spare = t.empty_like(grid.probes)
        for _ in range(int(bounces)):
            _, hits = self.light_probes_indirect(tables, settings, positions, grid, directions=directions, sets=sets, far=far,
                                                 strength=strength, out=spare)
            hits[masked] = abi.RM_RAY_INVALID
            nxt = LightGrid(self, spare, grid.origin, grid.step, grid.dims).set_depth(grid.depth, grid.normal_bias)
            grid, spare = nxt, grid.probes
        return grid

    def render_lit(self, tables, settings, W, H, grid, cameras=None, strength=1.0):
        """Frames lit by a LightGrid, bit-defined → float32 (N, H, W, 4), row 0 = bottom: camera_rays of every camera (None: the
        scene's own, N = 1) in tile_order through shade_rays_indirect — ONE launch per frame — and scattered back to their pixels
        on the device.  The successor of render_indirect: the albedo has the texture and the fractals' palette, and every word
        is defined by include/raymarcher_amd.h."""
        t = self.torch
        cams = [tables.camera] if cameras is None else cameras
        order = tile_order(W, H)
        where = t.from_numpy(order).to(self.device)
        out = t.empty((len(cams), H * W, 4), dtype=t.float32, device=self.device)
        for f, cam in enumerate(cams):
            out[f][where] = self.shade_rays_indirect(tables, settings, camera_rays(cam, W, H)[order], grid, far=cam.initialFar,
                                                     strength=strength)
        return out.view(len(cams), H, W, 4)

    def render_panorama(self, tables, settings, W, H, position, forward=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), far=None):
        """A W×H equirectangular panorama of the scene from `position` → float32 (H, W, 4), row 0 = bottom: panorama_rays shaded
        by shade_rays in tile_order (8×8 tiles: the rays of a wave are neighbours on the picture) and scattered back to their
        pixels on the device."""
        t = self.torch
        order = tile_order(W, H)
        colour = self.shade_rays(tables, settings, panorama_rays(position, W, H, forward, up)[order], far=far)
        out = t.empty((H * W, 4), dtype=t.float32, device=self.device)
        out[t.from_numpy(order).to(self.device)] = colour  # the inverse permutation: ray k is pixel order[k]
        return out.view(H, W, 4)

    def shade_rays_layers(self, tables, settings, rays, image_width, far=None, bright=False, out=None, out_bright=None):
        """rm_shade_rays_layers: shade_rays through terrain, sea and clouds (RM_FEAT_TERRAIN / SEA / CLOUD in `settings`), which
        shade_rays refuses → float32 (n, 4), or the pair (colour, bright).  image_width: the width in pixels of the image the rays
        belong to (a frame's W, a panorama's W; at least 1) — the sea normal's epsilon is divided by it and nothing else reads it.
        With RM_FEAT_CLOUD the march limit is the shader's 2000 and `far` is not read.  camera_rays of a frame with image_width = W
        give render()'s pixels bit for bit; without a layer bit the result is shade_rays'.  The definition is in
        include/raymarcher_amd.h."""
        t = self.torch
        rays = self._rays(rays)
        n = rays.shape[0]
        out = self._out(out, (n, 4), t.float32)
        bright = bright or out_bright is not None
        br = self._out(out_bright, (n, 4), t.float32, "out_bright") if bright else None
        res, _keep = self._resources(tables)
        check(lib().rm_shade_rays_layers(C.c_void_p(rays.data_ptr()), n, tables.camera.initialFar if far is None else far, image_width,
                                         tables.objects, tables.num_objects, tables.lights, tables.num_lights, C.byref(tables.globals_),
                                         C.byref(settings), C.byref(res), C.c_void_p(out.data_ptr()),
                                         C.c_void_p(br.data_ptr()) if bright else None, self._stream()))
        return (out, br) if bright else out

    def trace_rays_layers(self, tables, settings, rays, image_width, normals=True, out=None):
        """rm_trace_rays_layers: the closest VISIBLE SURFACE along arbitrary rays, the terrain and the sea included → (normal, t,
        position, object_id) as trace_rays returns them.  object_id: abi.RM_HIT_TERRAIN (−4) with the terrain's own surface normal,
        abi.RM_HIT_SEA (−3) with the shader's sea normal, else trace_rays' closest hit (an index, −1 a miss, abi.RM_RAY_INVALID).
        image_width as shade_rays_layers takes it; RM_FEAT_CLOUD is ignored (a volume has no closest hit).  normals=False: object_id
        and t only.  Occlusion through the layers is not defined: trace_rays has the objects' shadow march.  The definition is in
        include/raymarcher_amd.h."""
        t = self.torch
        rays = self._rays(rays)
        n = rays.shape[0]
        hits = self._out(out, (n, 8), t.float32)
        check(lib().rm_trace_rays_layers(C.c_void_p(rays.data_ptr()), n, image_width, tables.objects, tables.num_objects,
                                         C.byref(tables.globals_), C.byref(settings),
                                         abi.RM_TRACE_CLOSEST if normals else abi.RM_TRACE_NO_NORMAL, C.c_void_p(hits.data_ptr()),
                                         self._stream()))
        return hits[:, 0:3], hits[:, 3], hits[:, 4:7], hits[:, 7].view(t.int32)

    def order_rays(self, rays, origin_bits=7, dir_bits=8, sorted_rays=True, keys=False):
        """rm_rays_order: a coherence ordering of rays that come in no order, on the device → `order`, int32 (n,): order[k] is the
        input index of the ray at sorted position k.  After it, with sorted_rays (the default), the rays in that order, float32
        (n, 8) — rays[order] in every bit — and, with keys=True, the keys in INPUT order, int64 (n,) holding the uint64 bits: so the
        default is the pair (order, sorted), and with neither it is `order` alone.  rays as trace_rays takes them.  The key is the
        Morton code of the origin quantised to origin_bits (0 … 10) per axis over an octahedral map of the direction quantised to
        dir_bits (0 … 11), within the bounds of the call's rays; the order is the stable sort of the keys, rays with a non-finite
        component or a zero direction last.  tMax is not read.  Fewer bits are fewer sort passes (8 key bits each) and a coarser
        grouping: the defaults 7 and 8 (five passes) were as fast end to end as the finest key, 10 and 11 (seven passes), or
        faster, on seven of the eight tables of profiles/ray_order.md and 2 % slower on one; rays that all start at ONE point,
        and a camera's rays (whose origins on the near plane repeat what the directions say), do best with origin_bits=0 (three
        passes).  The definition is in include/raymarcher_amd.h."""
        t = self.torch
        rays = self._rays(rays)
        n = rays.shape[0]
        order = t.empty((n,), dtype=t.int32, device=self.device)
        srt = t.empty((n, 8), dtype=t.float32, device=self.device) if sorted_rays else None
        ks = t.empty((n,), dtype=t.int64, device=self.device) if keys else None
        check(lib().rm_rays_order(C.c_void_p(rays.data_ptr()), n, origin_bits, dir_bits, C.c_void_p(order.data_ptr()),
                                  C.c_void_p(srt.data_ptr()) if sorted_rays else None, C.c_void_p(ks.data_ptr()) if keys else None,
                                  self._stream()))
        extra = ([srt] if sorted_rays else []) + ([ks] if keys else [])
        return (order, *extra) if extra else order

    def restore_order(self, rows, order, out=None):
        """rm_rays_restore: results computed in sorted order back in the caller's order → out[order[k]] = rows[k], a tensor of
        rows' shape and dtype (`out`, if given; it may not be `rows`).  rows: a contiguous (n, 4) or (n, 8) tensor of a 4-byte dtype
        on this device — colours, RmRayHit or RmSurfacePoint rows; order: order_rays' int32 (n,).  An entry of `order` outside
        [0, n) is skipped; with a fresh `out` such a row is left uninitialised."""
        t = self.torch
        ok = t.is_tensor(rows) and rows.dim() == 2 and rows.shape[1] in (4, 8) and rows.element_size() == 4 and rows.is_contiguous() and \
            rows.device == self.device
        if not ok:
            raise ValueError(f"rows must be a contiguous (n, 4) or (n, 8) tensor of a 4-byte dtype on {self.device}")
        n = rows.shape[0]
        if not t.is_tensor(order) or tuple(order.shape) != (n,) or order.dtype != t.int32 or not order.is_contiguous() or order.device != self.device:
            raise ValueError(f"order must be a contiguous int32 tensor of shape ({n},) on {self.device}")
        out = self._out(out, rows.shape, rows.dtype)
        check(lib().rm_rays_restore(C.c_void_p(rows.data_ptr()), C.c_void_p(order.data_ptr()), n, 4 * rows.shape[1],
                                    C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def trace_rays_sorted(self, tables, settings, rays, mode="closest", normals=True, image_width=None, origin_bits=7, dir_bits=8):
        """trace_rays for rays in no order: order_rays, the trace on the sorted rays, restore_order → trace_rays' 4-tuple (normal, t,
        position, object_id) in the CALLER's order, the same bits trace_rays gives (a ray's result does not depend on which rays
        share its call), for the price of the sort instead of the price of incoherent waves.  With image_width the trace is
        trace_rays_layers (terrain and sea; mode "closest" only)."""
        t = self.torch
        if image_width is not None and mode != "closest":
            raise ValueError("with image_width (trace_rays_layers) the mode is 'closest'")
        order, srt = self.order_rays(rays, origin_bits, dir_bits)
        hits = t.empty((srt.shape[0], 8), dtype=t.float32, device=self.device)
        if image_width is None:
            self.trace_rays(tables, settings, srt, mode=mode, normals=normals, out=hits)
        else:
            self.trace_rays_layers(tables, settings, srt, image_width, normals=normals, out=hits)
        hits = self.restore_order(hits, order)
        return hits[:, 0:3], hits[:, 3], hits[:, 4:7], hits[:, 7].view(t.int32)

    def shade_rays_sorted(self, tables, settings, rays, far=None, bright=False, image_width=None, origin_bits=7, dir_bits=8):
        """shade_rays for rays in no order: order_rays, the shading of the sorted rays, restore_order → float32 (n, 4), or the pair
        (colour, bright) with bright=True, in the CALLER's order and the same bits shade_rays gives.  With image_width the shading
        is shade_rays_layers (terrain, sea and clouds)."""
        order, srt = self.order_rays(rays, origin_bits, dir_bits)
        if image_width is None:
            got = self.shade_rays(tables, settings, srt, far=far, bright=bright)
        else:
            got = self.shade_rays_layers(tables, settings, srt, image_width, far=far, bright=bright)
        if bright:
            return self.restore_order(got[0], order), self.restore_order(got[1], order)
        return self.restore_order(got, order)

    def render_panorama_layers(self, tables, settings, W, H, position, forward=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), far=None):
        """render_panorama through shade_rays_layers with image_width = W: a W×H equirectangular panorama with terrain, sea and
        clouds → float32 (H, W, 4), row 0 = bottom."""
        t = self.torch
        order = tile_order(W, H)
        colour = self.shade_rays_layers(tables, settings, panorama_rays(position, W, H, forward, up)[order], W, far=far)
        out = t.empty((H * W, 4), dtype=t.float32, device=self.device)
        out[t.from_numpy(order).to(self.device)] = colour  # the inverse permutation: ray k is pixel order[k]
        return out.view(H, W, 4)

    def sdf_grid(self, tables, settings, origin, step, dims, ids=False):
        """rm_sdf_grid: the scene's distance function on a dense lattice → float32 (nz, ny, nx), x fastest; with ids=True the pair
        (distances, int32 (nz, ny, nx) object indices).  Point (i, j, k) is origin + (i, j, k) · step in float32; dims = (nx, ny,
        nz).  The values are rm_probe_sdscene's minD and minObjIdx at those points; include/raymarcher_amd.h has the definition."""
        t = self.torch
        nx, ny, nz = (int(d) for d in dims)
        if min(nx, ny, nz) < 1:
            raise ValueError("every lattice dimension must be at least 1")
        dist = t.empty((nz, ny, nx), dtype=t.float32, device=self.device)
        obj = t.empty((nz, ny, nx), dtype=t.int32, device=self.device) if ids else None
        check(lib().rm_sdf_grid(tables.objects, tables.num_objects, C.byref(tables.globals_), C.byref(settings), _vec3(origin, "origin"),
                                _vec3(step, "step"), nx, ny, nz, C.c_void_p(dist.data_ptr()),
                                C.c_void_p(obj.data_ptr()) if ids else None, self._stream()))
        return (dist, obj) if ids else dist

    def extract_mesh(self, grid, origin, step, iso=0.0, ids=None):
        """rm_sdf_mesh: the quad mesh of the surface {grid = iso} by naive surface nets → (vertices float32 (n, 4), quads int32 (m,
        4)), and the vertices' object indices int32 (n) behind them when `ids` (the lattice's int32 indices, same shape) is given.
        grid: float32 (nz, ny, nx) on this device, from sdf_grid or from anywhere else.  A counting call, one read of two words,
        then an emitting call with exact capacities; raises if the two calls disagree about the counts."""
        t = self.torch
        if grid.dim() != 3 or grid.dtype != t.float32 or not grid.is_contiguous() or grid.device != self.device:
            raise ValueError(f"grid must be a contiguous float32 tensor of shape (nz, ny, nx) on {self.device}")
        if ids is not None and (tuple(ids.shape) != tuple(grid.shape) or ids.dtype != t.int32 or not ids.is_contiguous()
                                or ids.device != self.device):
            raise ValueError(f"ids must be a contiguous int32 tensor of shape {tuple(grid.shape)} on {self.device}")
        nz, ny, nx = grid.shape
        o, st = _vec3(origin, "origin"), _vec3(step, "step")
        idp = C.c_void_p(ids.data_ptr()) if ids is not None else None
        counts = t.zeros(2, dtype=t.int64, device=self.device)  # two uint32 words in the first eight bytes

        def call(max_v, max_q, v, vo, q):
            check(lib().rm_sdf_mesh(C.c_void_p(grid.data_ptr()), idp, nx, ny, nz, o, st, float(iso), max_v, max_q,
                                    C.c_void_p(v.data_ptr()) if v is not None else None,
                                    C.c_void_p(vo.data_ptr()) if vo is not None else None,
                                    C.c_void_p(q.data_ptr()) if q is not None else None, C.c_void_p(counts.data_ptr()), self._stream()))
            both = int(counts[0].item())
            return both & 0xFFFFFFFF, (both >> 32) & 0xFFFFFFFF

        nv, nq = call(0, 0, None, None, None)
        if nv > 2 ** 31 - 1 or nq > 2 ** 31 - 1:
            raise RaymarcherError(abi.RM_ERR_CAPACITY, f"{nv} vertices and {nq} quads exceed one call's capacity")
        verts = t.empty((nv, 4), dtype=t.float32, device=self.device)
        quads = t.empty((nq, 4), dtype=t.int32, device=self.device)
        vobj = t.empty((nv,), dtype=t.int32, device=self.device) if ids is not None else None
        if nv or nq:
            again = call(nv, nq, verts if nv else None, vobj if nv else None, quads if nq else None)
            if again != (nv, nq):
                raise RuntimeError(f"rm_sdf_mesh counted {(nv, nq)} vertices and quads, then {again}: the lattice changed between the calls")
        return (verts, quads, vobj) if ids is not None else (verts, quads)

    def scene_mesh(self, tables, settings, resolution, iso=0.001, bounds=None):
        """The scene's surface as a quad mesh: sdf_grid over the table's bounds, then extract_mesh → (vertices, quads, vertex object
        indices).  resolution: lattice points along the longest side of the bounds (at least 4); the step is the same on every axis
        and the lattice reaches one step past the bounds on every side, so a surface inside the bounds is closed.  iso: 0.001, the
        march's hit threshold — what the renderer shows as the surface, and the smallest value that has a Mandelbulb's inside.
        bounds: (lo, hi), or None for mesh_bounds(tables)."""
        return self._scene_mesh(tables, settings, resolution, iso, bounds)[:3]

    def _scene_mesh(self, tables, settings, resolution, iso, bounds):
        """scene_mesh's mesh and, behind it, the lattice step it chose."""
        origin, step, dims = self._scene_lattice(tables, resolution, bounds)
        dist, obj = self.sdf_grid(tables, settings, origin, (step,) * 3, dims, ids=True)
        return self.extract_mesh(dist, origin, (step,) * 3, iso, obj) + (step,)

    @staticmethod
    def _scene_lattice(tables, resolution, bounds):
        """The lattice scene_mesh lays over the bounds → (origin, step, dims)."""
        import numpy as np
        if int(resolution) < 4:
            raise ValueError("resolution must be at least 4")
        lo, hi = mesh_bounds(tables) if bounds is None else (np.asarray(b, dtype=np.float64) for b in bounds)
        lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        side = hi - lo
        if lo.shape != (3,) or hi.shape != (3,) or not np.isfinite(side).all() or not (side > 0).all():
            raise ValueError("bounds must be (lo, hi) with three finite components each and lo < hi")
        step = float(side.max()) / (int(resolution) - 3)
        dims = [min(int(resolution), int(np.ceil(sd / step)) + 3) for sd in side]
        return lo - step, step, dims

    # ---- block-sparse lattices: blocks of 8×8×8 cells, kept only where the surface passes (include/raymarcher_amd.h) ----
    @staticmethod
    def _blocks3(blocks):
        mx, my, mz = (int(b) for b in blocks)
        if min(mx, my, mz) < 1:
            raise ValueError("every block dimension must be at least 1")
        return mx, my, mz

    def _block_list(self, block_list):
        t = self.torch
        if (not t.is_tensor(block_list) or block_list.dim() != 2 or block_list.shape[1] != 4 or block_list.dtype != t.int32
                or not block_list.is_contiguous() or block_list.device != self.device):
            raise ValueError(f"block_list must be a contiguous int32 tensor of shape (n, 4) on {self.device}")
        return block_list

    def sdf_active_blocks(self, tables, settings, origin, step, blocks, iso):
        """rm_sdf_blocks_select: the blocks of the virtual lattice of blocks = (mx, my, mz) blocks — 8·m + 1 points per axis, point
        (i, j, k) at origin + (i, j, k) · step — whose 729 points are not all on one side of iso → int32 (n, 4) rows (bi, bj, bk,
        0) in linear order.  One call with a capacity guess, one more with the exact capacity if the count exceeded it."""
        return self._active_blocks(tables, settings, origin, step, blocks, iso, None)[0]

    def sdf_active_blocks_pruned(self, tables, settings, origin, step, blocks, iso, outside=4.0, inside=None):
        """rm_sdf_blocks_select_pruned: sdf_active_blocks without the evaluation of blocks far from the surface → (block_list,
        candidates).  The block corners are evaluated first; a block all of whose eight corners lie more than outside · h beyond
        iso, or more than inside · h below it (h: half a block's diagonal), is discarded unseen, the others — `candidates` of them —
        are decided exactly.  None means +inf: that side discards nothing.  The list is sdf_active_blocks' wherever the scene's
        distance function changes by at most outside (inside) per unit length on that side: a true distance does with 1; the inside
        of the fractal estimators honours no constant, which is why inside defaults to None, and the Mandelbulb's estimate on the
        outside exceeds the distance: on the 4097-point lattice of the headline bulb outside = 1 loses 16 of a million blocks and 2
        is the smallest value measured to lose none, so outside defaults to twice that (profiles/sdf_prune.md).  The same
        capacity-guess-then-exact protocol."""
        inf = float("inf")
        return self._active_blocks(tables, settings, origin, step, blocks, iso,
                                   (inf if outside is None else float(outside), inf if inside is None else float(inside)))

    def _active_blocks(self, tables, settings, origin, step, blocks, iso, prune):
        """The two selections' shared protocol → (block_list, candidates or None).  prune: None, or (lipschitzOut, lipschitzIn)."""
        t = self.torch
        mx, my, mz = self._blocks3(blocks)
        o, st = _vec3(origin, "origin"), _vec3(step, "step")
        count = t.zeros(2, dtype=t.int32, device=self.device)
        name = "rm_sdf_blocks_select" if prune is None else "rm_sdf_blocks_select_pruned"

        def call(capacity):
            out = t.empty((capacity, 4), dtype=t.int32, device=self.device)
            head = (tables.objects, tables.num_objects, C.byref(tables.globals_), C.byref(settings), o, st, mx, my, mz, float(iso))
            tail = (capacity, C.c_void_p(out.data_ptr()) if capacity else None, C.c_void_p(count.data_ptr()), self._stream())
            check(getattr(lib(), name)(*head, *(prune or ()), *tail))
            n, candidates = (int(x) & 0xFFFFFFFF for x in count.tolist())
            return out, n, candidates

        # a surface crosses about as many blocks as a few of the lattice's faces have
        guess = min(mx * my * mz, max(64, 4 * (mx * my + my * mz + mz * mx)))
        out, n, candidates = call(guess)
        if n > guess:
            if n > abi.RM_MAX_BLOCK_LIST:
                raise RaymarcherError(abi.RM_ERR_CAPACITY, f"{n} active blocks exceed RM_MAX_BLOCK_LIST: split the bounds")
            out, again, candidates = call(n)
            if again != n:
                raise RuntimeError(f"{name} counted {n} blocks, then {again}: the scene changed between the calls")
        return out[:n], (candidates if prune is not None else None)

    def sdf_grid_blocks(self, tables, settings, origin, step, blocks, block_list, ids=False):
        """rm_sdf_grid_blocks: the scene's distance function on the listed blocks only → float32 (n, 9, 9, 9), entry n's values as
        [c, b, a], x fastest; with ids=True the pair (distances, int32 object indices of the same shape).  The values are
        sdf_grid's at those lattice points; the slot of a void entry (outside the lattice, or a repeat) is left unwritten."""
        t = self.torch
        mx, my, mz = self._blocks3(blocks)
        bl = self._block_list(block_list)
        n = bl.shape[0]
        dist = t.empty((n, 9, 9, 9), dtype=t.float32, device=self.device)
        obj = t.empty((n, 9, 9, 9), dtype=t.int32, device=self.device) if ids else None
        check(lib().rm_sdf_grid_blocks(tables.objects, tables.num_objects, C.byref(tables.globals_), C.byref(settings), _vec3(origin, "origin"),
                                       _vec3(step, "step"), mx, my, mz, C.c_void_p(bl.data_ptr()) if n else None, n,
                                       C.c_void_p(dist.data_ptr()) if n else None, C.c_void_p(obj.data_ptr()) if ids and n else None,
                                       self._stream()))
        return (dist, obj) if ids else dist

    def extract_mesh_blocks(self, grid_blocks, block_list, blocks, origin, step, iso=0.0, ids=None):
        """rm_sdf_mesh_blocks: extract_mesh over a block list → (vertices float32 (n, 4), quads int32 (m, 4), open_vertices), with the
        vertices' object indices int32 (n) ahead of open_vertices when `ids` (int32, grid_blocks' shape) is given.  grid_blocks:
        float32 (n, 9, 9, 9) from sdf_grid_blocks.  open_vertices = 0: no quad of the dense mesh that touches a listed block is
        missing.  A counting call, one read of three words, then an emitting call with exact capacities; raises if the two disagree."""
        t = self.torch
        mx, my, mz = self._blocks3(blocks)
        bl = self._block_list(block_list)
        n = bl.shape[0]
        if (tuple(grid_blocks.shape) != (n, 9, 9, 9) or grid_blocks.dtype != t.float32 or not grid_blocks.is_contiguous()
                or grid_blocks.device != self.device):
            raise ValueError(f"grid_blocks must be a contiguous float32 tensor of shape ({n}, 9, 9, 9) on {self.device}")
        if ids is not None and (tuple(ids.shape) != (n, 9, 9, 9) or ids.dtype != t.int32 or not ids.is_contiguous() or ids.device != self.device):
            raise ValueError(f"ids must be a contiguous int32 tensor of shape ({n}, 9, 9, 9) on {self.device}")
        o, st = _vec3(origin, "origin"), _vec3(step, "step")
        counts = t.zeros(4, dtype=t.int32, device=self.device)

        def call(max_v, max_q, v, vo, q):
            check(lib().rm_sdf_mesh_blocks(C.c_void_p(grid_blocks.data_ptr()) if n else None, C.c_void_p(ids.data_ptr()) if ids is not None and n else None,
                                           C.c_void_p(bl.data_ptr()) if n else None, n, mx, my, mz, o, st, float(iso), max_v, max_q,
                                           C.c_void_p(v.data_ptr()) if v is not None else None,
                                           C.c_void_p(vo.data_ptr()) if vo is not None else None,
                                           C.c_void_p(q.data_ptr()) if q is not None else None, C.c_void_p(counts.data_ptr()), self._stream()))
            return tuple(int(x) & 0xFFFFFFFF for x in counts[:3].tolist())

        nv, nq, nopen = call(0, 0, None, None, None)
        if nv > 2 ** 31 - 1 or nq > 2 ** 31 - 1:
            raise RaymarcherError(abi.RM_ERR_CAPACITY, f"{nv} vertices and {nq} quads exceed one call's capacity")
        verts = t.empty((nv, 4), dtype=t.float32, device=self.device)
        quads = t.empty((nq, 4), dtype=t.int32, device=self.device)
        vobj = t.empty((nv,), dtype=t.int32, device=self.device) if ids is not None else None
        if nv or nq:
            again = call(nv, nq, verts if nv else None, vobj if nv else None, quads if nq else None)
            if again != (nv, nq, nopen):
                raise RuntimeError(f"rm_sdf_mesh_blocks counted {(nv, nq, nopen)}, then {again}: the blocks changed between the calls")
        return (verts, quads, vobj, nopen) if ids is not None else (verts, quads, nopen)

    def scene_mesh_sparse(self, tables, settings, resolution, iso=0.001, bounds=None):
        """scene_mesh beyond the dense lattice's limits: the active blocks of the lattice (sdf_active_blocks), the field on them
        (sdf_grid_blocks), the mesh over them (extract_mesh_blocks) → (vertices, quads, vertex object indices).  resolution (4 …
        4097), step and origin are scene_mesh's; the lattice has ceil((points − 1) / 8) blocks per axis, so it runs past the
        bounds on the high side.  The mesh is the dense mesh of that lattice."""
        return self._scene_mesh_sparse(tables, settings, resolution, iso, bounds)[:3]

    def _scene_mesh_sparse(self, tables, settings, resolution, iso, bounds, prune=None):
        """scene_mesh_sparse's mesh and, behind it, the lattice step it chose.  prune: None, or the (outside, inside) of
        sdf_active_blocks_pruned, which then selects the blocks."""
        if int(resolution) > 8 * abi.RM_MAX_LATTICE_BLOCKS + 1:
            raise ValueError("resolution must be at most 4097")
        origin, step, dims = self._scene_lattice(tables, resolution, bounds)
        blocks = [(d - 1 + 7) // 8 for d in dims]
        bl = self._select_blocks(tables, settings, origin, (step,) * 3, blocks, iso, prune)
        dist, obj = self.sdf_grid_blocks(tables, settings, origin, (step,) * 3, blocks, bl, ids=True)
        verts, quads, vobj, nopen = self.extract_mesh_blocks(dist, bl, blocks, origin, (step,) * 3, iso, obj)
        if nopen != 0:
            raise RuntimeError(f"{nopen} open vertices over the list of the lattice's own active blocks")
        return verts, quads, vobj, step

    def bake_mesh_sparse(self, tables, settings, resolution, iso=0.001, bounds=None, project=2, ao=True, colour=True):
        """bake_mesh on top of scene_mesh_sparse: the same outputs, resolution up to 4097."""
        return self._bake(tables, settings, self._scene_mesh_sparse(tables, settings, resolution, iso, bounds), iso, project, ao, colour)

    def _select_blocks(self, tables, settings, origin, step, blocks, iso, prune):
        """The block list of the *_sparse (prune None) and *_pruned (prune = (outside, inside)) methods."""
        if prune is None:
            return self.sdf_active_blocks(tables, settings, origin, step, blocks, iso)
        return self.sdf_active_blocks_pruned(tables, settings, origin, step, blocks, iso, *prune)[0]

    def scene_mesh_pruned(self, tables, settings, resolution, iso=0.001, bounds=None, outside=4.0, inside=None):
        """scene_mesh_sparse with the blocks selected by sdf_active_blocks_pruned(…, outside, inside): the same mesh wherever that
        list is sdf_active_blocks' (see there), without the sweep over every block of the lattice.  A list that lacks an active block
        cuts the mesh open: that raises, as in scene_mesh_sparse.  A list that lacks whole components of the surface does not."""
        return self._scene_mesh_sparse(tables, settings, resolution, iso, bounds, (outside, inside))[:3]

    def bake_mesh_pruned(self, tables, settings, resolution, iso=0.001, bounds=None, project=2, ao=True, colour=True, outside=4.0, inside=None):
        """bake_mesh_sparse on top of scene_mesh_pruned."""
        return self._bake(tables, settings, self._scene_mesh_sparse(tables, settings, resolution, iso, bounds, (outside, inside)), iso, project,
                          ao, colour)

    def bake_mesh_pruned_ambient(self, tables, settings, resolution, ambient=16, iso=0.001, bounds=None, project=2, ao=True, colour=True,
                                 outside=4.0, inside=None):
        """bake_mesh_pruned with a LatticeField.ambient pass of `ambient` hemisphere directions over it: the field is baked again with
        scene_field_pruned at the same resolution, the projected vertices and their normals go through ambient(directions=ambient),
        and the 8-bit colours are multiplied by its visibility (rounded to nearest) → bake_mesh_pruned's tuple with those colours.
        ambient=None, or colour=False, is bake_mesh_pruned as it is."""
        baked = self.bake_mesh_pruned(tables, settings, resolution, iso, bounds, project, ao, colour, outside, inside)
        if ambient is None or baked[5] is None:
            return baked
        t = self.torch
        verts, quads, object_id, normal, aos, rgb = baked
        dist, obj, bl, blocks, origin, step = self.scene_field_pruned(tables, settings, resolution, iso, bounds, outside, inside)
        with self.lattice_field_blocks(dist, bl, blocks, origin, step, obj) as field:
            visibility = field.ambient(verts, normal, directions=int(ambient), iso=iso)[1]
            shaded = t.clamp(t.round(rgb.to(t.float32) * visibility.clamp(0.0, 1.0)[:, None]), 0.0, 255.0).to(t.uint8)
            t.cuda.current_stream(self.device).synchronize()  # the handle is destroyed on the way out
        return verts, quads, object_id, normal, aos, shaded

    # ---- lattice queries: a baked lattice read back at points and marched by rays (include/raymarcher_amd.h) ----
    def _lattice(self, grid, ids, shape_text, shape_ok):
        t = self.torch
        if (not t.is_tensor(grid) or not shape_ok(grid) or grid.dtype != t.float32 or not grid.is_contiguous() or grid.device != self.device):
            raise ValueError(f"grid must be a contiguous float32 tensor of shape {shape_text} on {self.device}")
        if ids is not None and (not t.is_tensor(ids) or tuple(ids.shape) != tuple(grid.shape) or ids.dtype != t.int32
                                or not ids.is_contiguous() or ids.device != self.device):
            raise ValueError(f"ids must be a contiguous int32 tensor of shape {tuple(grid.shape)} on {self.device}")
        return C.c_void_p(grid.data_ptr()) if grid.numel() else None, C.c_void_p(ids.data_ptr()) if ids is not None and ids.numel() else None

    def sample_lattice(self, grid, origin, step, points, ids=None):
        """rm_sdf_sample: a dense lattice read back at arbitrary points, trilinearly → (gradient, value, cell, object_id): float32 (n,
        3) in world units, float32 (n), int32 (n, 3) and int32 (n), views of ONE float32 (n, 8) device tensor of RmFieldSample rows.
        grid: float32 (nz, ny, nx) on this device, from sdf_grid or from anywhere else, every dimension at least 2; ids: its int32
        object indices or None; points as shade_points takes them.  object_id: the id stored at the nearest corner of the point's
        cell (−1 without ids), abi.RM_FIELD_OUTSIDE for a point outside the lattice's box, abi.RM_RAY_INVALID for a non-finite
        point, both with zeros elsewhere.  The definition is in include/raymarcher_amd.h."""
        t = self.torch
        gp, ip = self._lattice(grid, ids, "(nz, ny, nx)", lambda g: g.dim() == 3)
        nz, ny, nx = grid.shape
        pts = self._points(points, "points")
        n = pts.shape[0]
        out = t.empty((n, 8), dtype=t.float32, device=self.device)
        check(lib().rm_sdf_sample(C.c_void_p(pts.data_ptr()) if n else None, n, gp, ip, nx, ny, nz, _vec3(origin, "origin"),
                                  _vec3(step, "step"), C.c_void_p(out.data_ptr()) if n else None, self._stream()))
        return out[:, 0:3], out[:, 3], out[:, 4:7].view(t.int32), out[:, 7].view(t.int32)

    def sample_lattice_blocks(self, grid_blocks, block_list, blocks, origin, step, points, ids=None):
        """rm_sdf_sample_blocks: sample_lattice on a block-sparse lattice → the same 4-tuple.  grid_blocks: float32 (n, 9, 9, 9) from
        sdf_grid_blocks, block_list its int32 (n, 4) list, blocks = (mx, my, mz), ids: int32 of grid_blocks' shape or None.  A point
        in a block the list does not name gets object_id abi.RM_FIELD_UNLISTED with its cell and zeros; everywhere else the record
        is sample_lattice's on the dense lattice in every bit."""
        t = self.torch
        mx, my, mz = self._blocks3(blocks)
        bl = self._block_list(block_list)
        nb = bl.shape[0]
        gp, ip = self._lattice(grid_blocks, ids, f"({nb}, 9, 9, 9)", lambda g: tuple(g.shape) == (nb, 9, 9, 9))
        pts = self._points(points, "points")
        n = pts.shape[0]
        out = t.empty((n, 8), dtype=t.float32, device=self.device)
        check(lib().rm_sdf_sample_blocks(C.c_void_p(pts.data_ptr()) if n else None, n, gp, ip,
                                         C.c_void_p(bl.data_ptr()) if nb else None, nb, mx, my, mz, _vec3(origin, "origin"),
                                         _vec3(step, "step"), C.c_void_p(out.data_ptr()) if n else None, self._stream()))
        return out[:, 0:3], out[:, 3], out[:, 4:7].view(t.int32), out[:, 7].view(t.int32)

    def trace_lattice(self, grid, origin, step, rays, iso=0.001, max_steps=256, ids=None, normals=True, out=None):
        """rm_sdf_trace: rays marched through a dense lattice instead of the scene → (normal, t, position, object_id) as trace_rays
        returns them, views of ONE float32 (n, 8) device tensor of RmRayHit rows (`out`, if given).  grid, ids as sample_lattice
        takes them, rays as trace_rays does.  A ray enters the lattice's box, steps by the interpolated value as the renderer's
        march steps by the distance, and hits at the first sample below iso: object_id = the id at the nearest corner (0 without
        ids), normal = the interpolant's normalised gradient; −1: a miss — the box or tMax left, or max_steps (at most
        abi.RM_MAX_FIELD_STEPS) used up — with t = tMax and zeros; abi.RM_RAY_INVALID as trace_rays has it.  normals=False leaves
        the point and the normal out (zeros).  The definition is in include/raymarcher_amd.h."""
        t = self.torch
        gp, ip = self._lattice(grid, ids, "(nz, ny, nx)", lambda g: g.dim() == 3)
        nz, ny, nx = grid.shape
        rays = self._rays(rays)
        n = rays.shape[0]
        hits = self._out(out, (n, 8), t.float32)
        check(lib().rm_sdf_trace(C.c_void_p(rays.data_ptr()) if n else None, n, gp, ip, nx, ny, nz, _vec3(origin, "origin"), _vec3(step, "step"),
                                 float(iso), int(max_steps), abi.RM_TRACE_CLOSEST if normals else abi.RM_TRACE_NO_NORMAL,
                                 C.c_void_p(hits.data_ptr()) if n else None, self._stream()))
        return hits[:, 0:3], hits[:, 3], hits[:, 4:7], hits[:, 7].view(t.int32)

    def trace_lattice_blocks(self, grid_blocks, block_list, blocks, origin, step, rays, iso=0.001, max_steps=256, ids=None, normals=True,
                             out=None):
        """rm_sdf_trace_blocks: trace_lattice through a block-sparse lattice → the same 4-tuple.  grid_blocks, block_list, blocks and
        ids as sample_lattice_blocks takes them.  A ray skips a block the list does not name in one step, to the face it leaves it
        through, so the march knows nothing of the inside of unlisted blocks: with scene_field_sparse's list (the blocks the
        surface passes through) a ray that starts outside the surface meets it where the dense march does; one that starts inside
        an object in an unlisted block reports the first listed sample below iso, not t = 0.  With every block listed the result
        is trace_lattice's in every bit."""
        t = self.torch
        mx, my, mz = self._blocks3(blocks)
        bl = self._block_list(block_list)
        nb = bl.shape[0]
        gp, ip = self._lattice(grid_blocks, ids, f"({nb}, 9, 9, 9)", lambda g: tuple(g.shape) == (nb, 9, 9, 9))
        rays = self._rays(rays)
        n = rays.shape[0]
        hits = self._out(out, (n, 8), t.float32)
        check(lib().rm_sdf_trace_blocks(C.c_void_p(rays.data_ptr()) if n else None, n, gp, ip,
                                        C.c_void_p(bl.data_ptr()) if nb else None, nb, mx, my, mz, _vec3(origin, "origin"), _vec3(step, "step"),
                                        float(iso), int(max_steps), abi.RM_TRACE_CLOSEST if normals else abi.RM_TRACE_NO_NORMAL,
                                        C.c_void_p(hits.data_ptr()) if n else None, self._stream()))
        return hits[:, 0:3], hits[:, 3], hits[:, 4:7], hits[:, 7].view(t.int32)

    def scene_field_sparse(self, tables, settings, resolution, iso=0.001, bounds=None):
        """The scene's distance field baked where its surface is, ready for sample_lattice_blocks and trace_lattice_blocks →
        (grid_blocks, ids, block_list, blocks, origin, step): scene_mesh_sparse's lattice (resolution 4 … 4097, the same step on
        every axis, returned as a 3-tuple), its active blocks at iso (sdf_active_blocks) and the field and object indices on them
        (sdf_grid_blocks)."""
        return self._scene_field_sparse(tables, settings, resolution, iso, bounds, None)

    def scene_field_pruned(self, tables, settings, resolution, iso=0.001, bounds=None, outside=4.0, inside=None):
        """scene_field_sparse with the blocks selected by sdf_active_blocks_pruned(…, outside, inside): cheap enough to bake a
        scene again when an object has moved."""
        return self._scene_field_sparse(tables, settings, resolution, iso, bounds, (outside, inside))

    def _scene_field_sparse(self, tables, settings, resolution, iso, bounds, prune):
        if int(resolution) > 8 * abi.RM_MAX_LATTICE_BLOCKS + 1:
            raise ValueError("resolution must be at most 4097")
        origin, step, dims = self._scene_lattice(tables, resolution, bounds)
        blocks = tuple((d - 1 + 7) // 8 for d in dims)
        bl = self._select_blocks(tables, settings, origin, (step,) * 3, blocks, iso, prune)
        dist, obj = self.sdf_grid_blocks(tables, settings, origin, (step,) * 3, blocks, bl, ids=True)
        return dist, obj, bl, blocks, origin, (step,) * 3

    # ---- lattice handles: what is derived from the block list built once (include/raymarcher_amd.h, "Lattice handles") ----
    def lattice_field(self, grid, origin, step, ids=None):
        """rm_field_create: a handle on a dense lattice → LatticeField.  grid, ids as sample_lattice takes them; the handle borrows
        them (the LatticeField keeps references) and reads their values as they are when a query runs."""
        gp, ip = self._lattice(grid, ids, "(nz, ny, nx)", lambda g: g.dim() == 3)
        nz, ny, nx = grid.shape
        h = C.c_void_p()
        check(lib().rm_field_create(gp, ip, nx, ny, nz, _vec3(origin, "origin"), _vec3(step, "step"), C.byref(h)))
        return LatticeField(self, h, (grid, ids), (tuple(origin), tuple(step), (nx - 1, ny - 1, nz - 1)))

    def lattice_field_blocks(self, grid_blocks, block_list, blocks, origin, step, ids=None):
        """rm_field_create_blocks: a handle on a block-sparse lattice → LatticeField.  grid_blocks, block_list, blocks and ids as
        sample_lattice_blocks takes them.  The block map and the coarse level are built here, once, on the current stream, which is
        synchronised; block_list is not needed afterwards, grid_blocks and ids are borrowed as lattice_field borrows."""
        mx, my, mz = self._blocks3(blocks)
        bl = self._block_list(block_list)
        nb = bl.shape[0]
        gp, ip = self._lattice(grid_blocks, ids, f"({nb}, 9, 9, 9)", lambda g: tuple(g.shape) == (nb, 9, 9, 9))
        h = C.c_void_p()
        check(lib().rm_field_create_blocks(gp, ip, C.c_void_p(bl.data_ptr()) if nb else None, nb, mx, my, mz, _vec3(origin, "origin"),
                                           _vec3(step, "step"), self._stream(), C.byref(h)))
        return LatticeField(self, h, (grid_blocks, ids), (tuple(origin), tuple(step), (8 * mx, 8 * my, 8 * mz)))

    def scene_field(self, tables, settings, resolution, iso=0.001, bounds=None):
        """scene_field_sparse's lattice behind a handle → LatticeField: the scene's distance field baked where its surface is, ready
        for sample and trace, occlusion marches included."""
        dist, obj, bl, blocks, origin, step = self.scene_field_sparse(tables, settings, resolution, iso, bounds)
        return self.lattice_field_blocks(dist, bl, blocks, origin, step, obj)

    def shade_points(self, tables, settings, points, view=None, far=None, colour=True, ao=False, project=0, iso=0.001,
                     max_move=float("inf")):
        """rm_shade_points: what the renderer thinks of points the caller already has, one lane per point in one launch → (normal,
        distance, position, object_id, ao or None, colour or None): float32 (n, 3), (n), (n, 3) and int32 (n), views of ONE float32
        (n, 8) device tensor of RmSurfacePoint rows; float32 (n) with ao=True; float32 (n, 4) with colour=True.  points: float32
        (n, 3) or (n, 4) (scene_mesh's vertices as they are; the fourth is not read), view: the same shapes or None — numpy arrays,
        which are uploaded, or tensors on this device.  project: steps that move each point onto the surface {distance = iso}
        before anything is evaluated, none of them farther than max_move from where the point began; position is where it ended.
        object_id −1: no object there (zeros everywhere); abi.RM_RAY_INVALID: a non-finite point or a non-finite or zero view.
        colour: render()'s shading at the point — materials, textures, trap palettes, shadows from the scene's lights, no reflection
        or refraction — seen along view, or head-on (−normal) without one; far (None = tables.camera.initialFar): the shadow
        marches' limit.  ao: calcAO at the point whatever settings.enableAmbientOcclusion says.  The definition is in
        include/raymarcher_amd.h."""
        t = self.torch
        pts = self._points(points, "points")
        n = pts.shape[0]
        vw = None if view is None else self._points(view, "view")
        if vw is not None and vw.shape[0] != n:
            raise ValueError("one view direction per point")
        ps = abi.RmPointsSettings(tables.camera.initialFar if far is None else far, iso, max_move, int(project))
        surface = t.empty((n, 8), dtype=t.float32, device=self.device)
        aos = t.empty((n,), dtype=t.float32, device=self.device) if ao else None
        col = t.empty((n, 4), dtype=t.float32, device=self.device) if colour else None
        res, _keep = self._resources(tables)
        check(lib().rm_shade_points(C.c_void_p(pts.data_ptr()), C.c_void_p(vw.data_ptr()) if vw is not None else None, n, C.byref(ps),
                                    tables.objects, tables.num_objects, tables.lights, tables.num_lights, C.byref(tables.globals_),
                                    C.byref(settings), C.byref(res), C.c_void_p(surface.data_ptr()),
                                    C.c_void_p(aos.data_ptr()) if ao else None, C.c_void_p(col.data_ptr()) if colour else None,
                                    self._stream()))
        return surface[:, 0:3], surface[:, 3], surface[:, 4:7], surface[:, 7].view(t.int32), aos, col

    def _points(self, a, name):
        """`a` as shade_points takes points and views: (n, 3) or (n, 4) float32, uploaded if it is a numpy array → a contiguous
        (n, 4) tensor on this device (an (n, 4) tensor that is one already is used in place)."""
        t = self.torch
        if not t.is_tensor(a):
            import numpy as np
            a = t.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        if a.dim() != 2 or a.shape[1] not in (3, 4) or a.dtype != t.float32:
            raise ValueError(f"{name} must be float32 of shape (n, 3) or (n, 4)")
        a = a.to(self.device)
        if a.shape[1] == 3:
            a = t.cat([a, t.zeros((a.shape[0], 1), dtype=t.float32, device=self.device)], dim=1)
        return a.contiguous()

    def bake_mesh(self, tables, settings, resolution, iso=0.001, bounds=None, project=2, ao=True, colour=True):
        """scene_mesh with everything a DCC tool wants on its vertices → (vertices float32 (n, 4), quads int32 (m, 4), object indices
        int32 (n), normals float32 (n, 3), ao float32 (n) or None, colours uint8 (n, 3) or None).  The mesh is scene_mesh's; its
        vertices then go through shade_points with `project` steps onto {distance = iso}, none farther than half the diagonal of a
        lattice cell from where surface nets put it, so a vertex stays near its cell; the vertices returned are the projected ones
        (w = 0) and the object indices are sdScene's at them.  Colours are the view-independent bake (each vertex seen head-on)
        through to_rgba8, the library's one float → 8-bit conversion.  write_ply_ex takes the result as it is."""
        return self._bake(tables, settings, self._scene_mesh(tables, settings, resolution, iso, bounds), iso, project, ao, colour)

    def _bake(self, tables, settings, mesh, iso, project, ao, colour):
        """bake_mesh behind its mesh: (vertices, quads, vertex objects, step) of _scene_mesh or _scene_mesh_sparse."""
        t = self.torch
        verts, quads, _vobj, step = mesh
        normal, _d, position, object_id, aos, col = self.shade_points(tables, settings, verts, colour=colour, ao=ao, project=project,
                                                                        iso=iso, max_move=0.5 * step * 3.0 ** 0.5)
        n = verts.shape[0]
        out = t.zeros((n, 4), dtype=t.float32, device=self.device)
        out[:, 0:3] = position
        rgb = None
        if colour:  # the n colours as one row of a frame: a single row has nothing to flip
            rgb = self.to_rgba8(col.view(1, n, 4))[0, :, 0:3].contiguous() if n else t.empty((0, 3), dtype=t.uint8, device=self.device)
        return out, quads, object_id.contiguous(), normal.contiguous(), aos, rgb

    def pick(self, tables, settings, W, H, x, y, camera=None):
        """What lies under pixel (x, y) of a W×H frame (y = 0 the bottom row) → (object_id, position, normal, t): an int (−1: nothing),
        two tuples of three floats and a float, through camera_rays and trace_rays — the values rm_render_gbuffer has for that
        pixel.  camera: None (the scene's own) or an RmCamera.  It waits for the result."""
        ray = camera_rays(tables.camera if camera is None else camera, W, H, [(x, y)])
        normal, t, position, object_id = self.trace_rays(tables, settings, ray)
        return (int(object_id[0]), tuple(position[0].tolist()), tuple(normal[0].tolist()), float(t[0]))

    def render_counted(self, tables, settings, W, H, mode=abi.RM_COUNT_REFERENCE):
        """rm_render_counted_res: the frame plus its work counters — the reference's work (mode RM_COUNT_REFERENCE) or
        what the production kernel really executes (RM_COUNT_EXECUTED; plain scene classes only)."""
        t = self.torch
        out = t.empty((H, W, 4), dtype=t.float32, device=self.device)
        cnt = abi.RmCounters()
        res, _keep = self._resources(tables)
        t.cuda.synchronize(self.device)
        check(lib().rm_render_counted_res(*tables.args(settings), C.byref(res), W, H, 0, H, C.c_void_p(out.data_ptr()), None, mode,
                                          C.byref(cnt)))
        return out, cnt

    def render_clocked(self, tables, settings, W, H, wave_spans=False):
        """rm_render_clocked: the frame from the stamped diagnostic build and the shader clock (MHz) it ran at; with
        wave_spans=True also an int64 tensor (waves, 2) of every wave's first / last 100 MHz tick."""
        t = self.torch
        out = t.empty((H, W, 4), dtype=t.float32, device=self.device)
        mhz = C.c_double()
        # one (first, last) pair per wave; the kernel indexes tile·(waves per workgroup) + wave with tiles = ceil(W / (8·wpb)) per
        # row, so a row holds at most ceil(W/8) + 3 waves for any RM_WAVES_PER_BLOCK in {1, 2, 4}
        spans = t.zeros(((((W + 7) // 8) + 3) * ((H + 7) // 8), 2), dtype=t.int64, device=self.device) if wave_spans else None
        t.cuda.synchronize(self.device)
        check(lib().rm_render_clocked(*tables.args(settings), W, H, C.c_void_p(out.data_ptr()), C.byref(mhz),
                                      C.c_void_p(spans.data_ptr()) if wave_spans else None))
        return (out, mhz.value, spans) if wave_spans else (out, mhz.value)

    def render_tiles(self, tables, settings, W, H, tile_rows, shard, num_shards, out=None):
        """rm_render_tiles: this shard's interleaved row tiles, packed → (rm_shard_rows, W, 4)."""
        t = self.torch
        n = lib().rm_shard_rows(H, tile_rows, shard, num_shards)
        out = self._out(out, (max(n, 0), W, 4), t.float32)
        res, _keep = self._resources(tables)
        check(lib().rm_render_tiles_res(*tables.args(settings), C.byref(res), W, H, tile_rows, shard, num_shards,
                                        C.c_void_p(out.data_ptr()), None, self._stream()))
        return out

    def deinterleave(self, gathered, W, H, tile_rows, num_shards, shard_stride_rows=0, out=None):
        t = self.torch
        frame = self._out(out, (H, W, 4), t.float32)
        check(lib().rm_deinterleave(C.c_void_p(gathered.data_ptr()), C.c_void_p(frame.data_ptr()), W, H, tile_rows,
                                    num_shards, shard_stride_rows, self._stream()))
        return frame

    def tiles_to_rgba8(self, tiles, out=None):
        """rm_tiles_to_rgba8: a shard's packed float4 rows → RGBA8, same rows (clamp → ×255 → round, no flip)."""
        t = self.torch
        rows, W = tiles.shape[0], tiles.shape[1]
        out = self._out(out, (rows, W, 4), t.uint8)
        check(lib().rm_tiles_to_rgba8(C.c_void_p(tiles.data_ptr()), C.c_void_p(out.data_ptr()), W, rows, self._stream()))
        return out

    def deinterleave_rgba8(self, gathered8, W, H, tile_rows, num_shards, shard_stride_rows=0, flip=True, out=None):
        """rm_deinterleave_rgba8: gathered RGBA8 slots → the frame's image (flip: row 0 = top, as to_rgba8 writes it)."""
        t = self.torch
        img = self._out(out, (H, W, 4), t.uint8)
        check(lib().rm_deinterleave_rgba8(C.c_void_p(gathered8.data_ptr()), C.c_void_p(img.data_ptr()), W, H, tile_rows, num_shards,
                                          shard_stride_rows, 1 if flip else 0, self._stream()))
        return img

    def post_process(self, frame, bright, post, out=None):
        """rm_post_process: bloom / HDR / gamma / FXAA (applyLightEffects + applyFXAA, realtimerender.cpp:78-165)."""
        t = self.torch
        H, W = frame.shape[0], frame.shape[1]
        out = self._out(out, (H, W, 4), t.float32)
        check(lib().rm_post_process(C.c_void_p(frame.data_ptr()), C.c_void_p(bright.data_ptr()) if bright is not None else None,
                                    C.c_void_p(out.data_ptr()), W, H, C.byref(post), self._stream()))
        return out

    def to_rgba8(self, frame, out=None):
        """Clamp/quantise + vertical flip (saveViewportImage, realtime.cpp:284-350) → uint8 (H, W, 4)."""
        t = self.torch
        H, W = frame.shape[0], frame.shape[1]
        out = self._out(out, (H, W, 4), t.uint8)
        check(lib().rm_frame_to_rgba8(C.c_void_p(frame.data_ptr()), C.c_void_p(out.data_ptr()), W, H, self._stream()))
        return out

    def _frames(self, frames, name):
        """(N, H, W) of a batch of frames (N, H, W, 4); ValueError for anything else.  Type and device: _out."""
        if not isinstance(frames, self.torch.Tensor) or frames.dim() != 4 or frames.shape[-1] != 4:
            raise ValueError(f"{name} must be a tensor of shape (N, H, W, 4)")
        n, H, W = (int(d) for d in frames.shape[:3])
        if n > abi.RM_MAX_BATCH_FRAMES:
            raise ValueError(f"{n} frames: at most RM_MAX_BATCH_FRAMES = {abi.RM_MAX_BATCH_FRAMES} frames per batch")
        return n, H, W

    def post_process_batch(self, frames, brights, post, out=None):
        """rm_post_process_batch: post_process of every frame of (N, H, W, 4) float32 `frames` (row 0 = bottom), brights the
        matching BrightColor planes (None without bloom).  post: one RmPostSettings for every frame, or a sequence of N with the
        same enable flags (the exposure may differ).  out may be `frames` itself (in place)."""
        t = self.torch
        n, H, W = self._frames(frames, "frames")
        ps = post_array(post, n)
        self._out(frames, (n, H, W, 4), t.float32, "frames")
        if brights is not None:
            self._out(brights, (n, H, W, 4), t.float32, "brights")
        elif ps[0].enableBloom:
            raise ValueError("bloom needs the BrightColor planes (brights)")
        out = self._out(out, (n, H, W, 4), t.float32)
        check(lib().rm_post_process_batch(C.c_void_p(frames.data_ptr()), C.c_void_p(brights.data_ptr()) if brights is not None else None,
                                          C.c_void_p(out.data_ptr()), W, H, n, ps, len(ps), self._stream()))
        return out

    def to_rgba8_batch(self, frames, out=None):
        """rm_frames_to_rgba8: to_rgba8 of every frame of (N, H, W, 4) float32 `frames` → uint8 (N, H, W, 4), each image's top
        row first."""
        t = self.torch
        n, H, W = self._frames(frames, "frames")
        self._out(frames, (n, H, W, 4), t.float32, "frames")
        out = self._out(out, (n, H, W, 4), t.uint8)
        check(lib().rm_frames_to_rgba8(C.c_void_p(frames.data_ptr()), C.c_void_p(out.data_ptr()), W, H, n, self._stream()))
        return out

    def render_sequence(self, tables, settings, W, H, cameras, globals_=None, post=None, supersample=1, adaptive=None, accumulate=None,
                        *, objects=None, lights=None):
        """The finished images of an exported sequence: render_batch (with the BrightColor planes only when bloom is on), then
        post_process_batch in place (skipped for post=None), then to_rgba8_batch → uint8 (N, H, W, 4), each image's top row
        first.  post: one RmPostSettings or a sequence of N (see post_process_batch).  supersample = 2 or 4: the render step is
        render_supersampled with that many samples per pixel along each axis (bloom then sees the resolved BrightColor).
        adaptive = t: the render step is render_adaptive(…, supersample, t) — those samples only where the 1-sample frame shows
        contrast above t.  accumulate = n: the render step is render_accumulated(…, n) — len(cameras) / n images, each the mean of n
        consecutive cameras (and globals); not together with supersample > 1 or adaptive.  objects / lights: per-camera object /
        light tables (render_animated's arguments) — the render step is then render_animated(…, accumulate or 1, objects, lights);
        not together with supersample > 1 or adaptive either."""
        animated = objects is not None or lights is not None
        if animated and (supersample != 1 or adaptive is not None):
            raise ValueError("objects / lights cannot be combined with supersample > 1 or adaptive")
        if accumulate is not None and (supersample != 1 or adaptive is not None):
            raise ValueError("accumulate cannot be combined with supersample > 1 or adaptive")
        if accumulate is not None and (not isinstance(accumulate, int) or accumulate < 1 or len(cameras) % accumulate):
            raise ValueError(f"accumulate = {accumulate!r}: a positive integer that divides the {len(cameras)} cameras")
        ps = post_array(post, len(cameras) // (accumulate or 1)) if post is not None else None
        bloom = ps is not None and bool(ps[0].enableBloom)
        if animated:
            frames = self.render_animated(tables, settings, W, H, cameras, accumulate or 1, objects, lights, globals_, bright=bloom)
        elif accumulate is not None:
            frames = self.render_accumulated(tables, settings, W, H, cameras, accumulate, globals_, bright=bloom)
        elif adaptive is not None:
            frames = self.render_adaptive(tables, settings, W, H, cameras, supersample, adaptive, globals_, bright=bloom)
        elif supersample == 1:
            frames = self.render_batch(tables, settings, W, H, cameras, globals_, bright=bloom)
        else:
            frames = self.render_supersampled(tables, settings, W, H, cameras, supersample, globals_, bright=bloom)
        brights = None
        if bloom:
            frames, brights = frames
        if ps is not None:
            self.post_process_batch(frames, brights, post, out=frames)
        return self.to_rgba8_batch(frames)

    def save_png(self, frame, path):
        img = self.to_rgba8(frame).cpu().contiguous()
        check(lib().rm_write_png(str(path).encode(), C.c_void_p(img.data_ptr()), img.shape[1], img.shape[0]))

    def probe_math(self, fn, x, y=None, z=None, out=None):
        t = self.torch
        out = t.empty_like(x) if out is None else self._out(out, x.shape, x.dtype)
        check(lib().rm_probe_math(fn, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()) if y is not None else None,
                                  C.c_void_p(z.data_ptr()) if z is not None else None, C.c_void_p(out.data_ptr()),
                                  x.numel(), self._stream()))
        return out

    def probe_sdscene(self, tables, settings, pts, out=None):
        t = self.torch
        n = pts.shape[0]
        out = self._out(out, (n, 4), t.float32)
        check(lib().rm_probe_sdscene(tables.objects, tables.num_objects, C.byref(tables.globals_), C.byref(settings),
                                     C.c_void_p(pts.data_ptr()), C.c_void_p(out.data_ptr()), n, self._stream()))
        return out

    def probe_bump(self, pts, out=None):
        """The four noise samples of the bump gradient at the (n, 3) points `pts` (include/raymarcher_amd.h, rm_probe_bump; point i
        runs on lane i % 64 of wave i / 64).  Returns (n, 4): nv, g0, g1, g2."""
        t = self.torch
        n = pts.shape[0]
        if tuple(pts.shape) != (n, 3) or pts.dtype != t.float32 or not pts.is_contiguous() or pts.device != self.device:
            raise ValueError(f"pts must be a contiguous float32 tensor of shape (n, 3) on {self.device}")
        out = self._out(out, (n, 4), t.float32)
        check(lib().rm_probe_bump(C.c_void_p(pts.data_ptr()), C.c_void_p(out.data_ptr()), n, self._stream()))
        return out

    def probe_sdscene_variant(self, tables, settings, pts, bulb_class=0, count=0, trap=1, skip=0, track=0, one=-1, ub=None,
                              out=None):
        """One production instantiation of the scene evaluator at the (n, 3) points `pts` (include/raymarcher_amd.h,
        rm_probe_sdscene_variant; point i runs on lane i % 64 of wave i / 64).  ub: (n,) upper bounds of the minimum or None
        (+inf).  Returns (n, 8): d, idx, trap.x, trap.y, trap.z, trap.w, second, shapes evaluated."""
        t = self.torch
        n = pts.shape[0]
        if tuple(pts.shape) != (n, 3) or pts.dtype != t.float32 or not pts.is_contiguous() or pts.device != self.device:
            raise ValueError(f"pts must be a contiguous float32 tensor of shape (n, 3) on {self.device}")
        if ub is not None and (tuple(ub.shape) != (n,) or ub.dtype != t.float32 or not ub.is_contiguous() or ub.device != self.device):
            raise ValueError(f"ub must be a contiguous float32 tensor of shape ({n},) on {self.device}")
        out = self._out(out, (n, 8), t.float32)
        check(lib().rm_probe_sdscene_variant(tables.objects, tables.num_objects, C.byref(tables.globals_), C.byref(settings),
                                             bulb_class, count, trap, skip, track, one, C.c_void_p(pts.data_ptr()),
                                             C.c_void_p(ub.data_ptr()) if ub is not None else None,
                                             C.c_void_p(out.data_ptr()), n, self._stream()))
        return out

    def probe_pool_cull(self, tables, settings, pts, bulb_class, light, far, out=None):
        """The shadow pool's cull end for the (n, 3) shadow origins `pts` and directional light `light` (include/raymarcher_amd.h,
        rm_probe_pool_cull; point i runs on lane i % 64 of wave i / 64).  Returns (n, 8): end and own from the staged constants,
        end and own from the whole computation, the direction normalised on the device, 0."""
        t = self.torch
        n = pts.shape[0]
        if tuple(pts.shape) != (n, 3) or pts.dtype != t.float32 or not pts.is_contiguous() or pts.device != self.device:
            raise ValueError(f"pts must be a contiguous float32 tensor of shape (n, 3) on {self.device}")
        out = self._out(out, (n, 8), t.float32)
        check(lib().rm_probe_pool_cull(tables.objects, tables.num_objects, tables.lights, tables.num_lights, C.byref(tables.globals_),
                                       C.byref(settings), bulb_class, light, far, C.c_void_p(pts.data_ptr()),
                                       C.c_void_p(out.data_ptr()), n, self._stream()))
        return out
