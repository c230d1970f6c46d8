"""intrinsicnerf_amd - MI355X (gfx950) implementation of IntrinsicNeRF's volumetric render_rays hot path.

  object_level   drop-in for object_level/run_nerf.py + run_nerf_helpers.py (render, render_rays, ...)
  ssr            drop-in for SSR/ + train_SSR_main.py's render path (SSRRenderMixin, Semantic_NeRF, ...)
  losses         the trainers' loss terms, one forward and one backward launch (compute_intrinsic_loss, *_step_loss)
  geometry       mesh extraction: query lattice, occupancy grid, marching cubes, normals, cleaning, vertex rays, 8-bit vertex colours and
                 the PLY (grid_within_bound, make_3D_grid, occupancy_grid, marching_cubes, vertex_normals, clean_mesh, extract_mesh,
                 vertex_rays, vertex_colours, write_ply)
  evaluation     the trainer's validation metrics on the device (calculate_segmentation_metrics, calculate_depth_metrics, FrameEvaluator)
  optim          the trainers' optimizer.step(): Adam as one launch of the library (optim.Adam)
  draws          the training step's random variates drawn in the kernels (DrawState; opt-in)
  kernels        tensor-level launchers of the C ABI (include/inerf.h, libinerf.so)
  packing        state dict -> MFMA-fragment-ordered weight blob
  distributed    ray sharding across the GPUs of a node + RCCL gather of the rendered maps

The arithmetic lives in ``libinerf.so`` (hand-written HIP, built by ``intrinsicnerf_amd._build`` /
``__graft_entry__.build()``).  There is no CPU, eager or oracle fallback: without the library and a HIP
device the render entry points raise.
"""
from . import _capi, kernels, packing  # noqa: F401
from . import object_level, ssr  # noqa: F401
from . import geometry  # noqa: F401
from . import evaluation  # noqa: F401
from . import optim  # noqa: F401
from . import draws  # noqa: F401
from .draws import DrawState  # noqa: F401
from .optim import Adam  # noqa: F401

__version__ = "0.1.0"
