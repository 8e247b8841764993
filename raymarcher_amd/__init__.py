"""raymarcher_amd — MI355X-native sphere-tracing renderer (HIP kernels behind a C-ABI).

Python here is plumbing: ctypes bindings of include/raymarcher_amd.h, torch for device memory /
streams / torch.distributed.  The renderer itself is raymarcher_amd/lib/libraymarcher_amd.so.
"""
from . import abi  # noqa: F401
from ._lib import LIB_PATH, RaymarcherError, lib  # noqa: F401
from .render import (LatticeField, Renderer, Scene, SceneTables, camera_rays, hemisphere_directions, mesh_bounds, panorama_rays, sh_irradiance, sphere_directions, tile_order,  # noqa: F401
                     translated_objects, write_ply, write_ply_ex)
