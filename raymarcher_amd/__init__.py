"""raymarcher_amd — MI355X-native sphere-tracing renderer (HIP kernels behind a C-ABI).

Python here is plumbing: ctypes bindings of include/raymarcher_amd.h, torch for device memory /
streams / torch.distributed.  The renderer itself is raymarcher_amd/lib/libraymarcher_amd.so.
"""
from . import abi  # noqa: F401
from ._lib import LIB_PATH, RaymarcherError, lib  # noqa: F401
from .render import (LatticeField, LightGrid, Renderer, Scene, SceneTables, camera_rays, hemisphere_directions, light_grid_positions, mesh_bounds, panorama_rays, probe_depth_weights,  # noqa: F401
                     sh_irradiance, sphere_directions, tile_order, translated_objects, write_ply, write_ply_ex)
