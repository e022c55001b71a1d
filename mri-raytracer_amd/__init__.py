"""mrirt — MI355X-native MRI volume ray-marcher (drop-in for the reference's render call).

The importable name is ``mrirt`` (see ``mrirt.py`` at the repo root); this directory carries
the task-mandated name ``mri-raytracer_amd``.  Layout:
  csrc/       hand-written gfx950 HIP kernels + the C ABI (include/mrirt.h) -> libmrirt.so
  _lib.py     ctypes binding (fails loudly when the library is missing — no CPU fallback)
  render.py   render_brats / render_volume_u8 / render_sdf over device tensors
  transfer.py RGBA transfer-function tables for render_brats(tf=...): tf_ramp, tf_from_points, tf_preset
  grad.py     K1 backward: render_brats_backward, render_brats_autograd (frame gradients to voxels and window / level)
  soft.py     the soft prediction overlay: render_brats_soft, its backward and render_brats_soft_autograd (frame gradients to logits)
  mesh.py     K4: PLY loading, the reference's BVH, upload + validation, render_mesh; class surfaces of label volumes
  components.py  connected components of label volumes, their sizes, small-component removal, slice counts (csrc/components.hip)
  shim.py     slangpy-shaped ``Device`` / ``ComputeKernel.dispatch(thread_count, vars, ...)``
  camera.py   OrbitalCamera (both reference variants)
  volume.py   load-time volume preparation (normalise, flatten, world frame, u8 pack, BC4) and the same on the device
              (normalize_intensity_device, zscore_nonzero_device, gaussian_filter_device: csrc/prep.hip)
  inr.py      model_load / build_input / apply_mlp / predict_volume on the MFMA MLP kernel
  tiles.py    image-tile sharding + RCCL framebuffer gather (one process per GPU)
  synth.py    deterministic synthetic scenes for tests and bench
"""
from . import _lib, camera, components, grad, inr, mesh, nifti, params, render, shim, soft, synth, tiles, torch_ops, transfer, viewer, volume  # noqa: F401
from .transfer import tf_from_points, tf_preset, tf_ramp  # noqa: F401
from .camera import OrbitalCamera  # noqa: F401
from .components import component_sizes, label_components, remove_small_components, slice_counts  # noqa: F401
from .grad import render_brats_autograd, render_brats_backward  # noqa: F401
from .inr import apply_mlp, build_input, compute_multi_metrics, inr_forward, model_load, predict_volume, prepare_case, render_brats_inr  # noqa: F401
from .inr import (boundary_weights, compute_uncertainty_mc_dropout, inject_desc, inject_dropout, inject_forward, inject_load,  # noqa: F401
                  predict_full_volume)
from .mesh import (build_bvh, extract_surface, load_ply, normalize_mesh, render_mesh, surface_mesh,  # noqa: F401
                   upload_mesh)
from .shim import Device, KernelShim  # noqa: F401
from .volume import gaussian_filter_device, normalize_intensity_device, zscore_nonzero_device  # noqa: F401
from .soft import render_brats_soft, render_brats_soft_autograd, render_brats_soft_backward  # noqa: F401
from .render import (Grid, detile, render_brats, render_sdf, render_volume_u8, tiles_for_rank,  # noqa: F401
                     unbrick_grid, upload_grid, upload_label_cells, upload_mod4)

__version__ = "0.1.0"
