"""nerf-rs_amd: MI355X-native drop-in for the hot path of elisabeth96/nerf-rs.

Python host mirror of the reference's interface for this path (same names, argument meaning and error behaviour),
sitting on top of the C ABI of libnerf_mi355x.so (include/nerf_mi355x.h).  PyTorch is optional plumbing only
(device buffers, streams, torch.distributed over RCCL for the framebuffer gather).
"""
from ._lib import NerfError, build_native, lib_path, load_library  # noqa: F401
from .api import (Camera, Component, Mesh, Network, RenderOpts, Renderer, Stats, band_row_indices, band_rows, camera_from_pose, camera_from_samples,  # noqa: F401
                  isosurface, lattice_components, lattice_components_device, load_network_blob, load_network_from_dir, pack_network_dir, quantize_rgb8, quantize_rgba8, render_image, render_image_multi, render_image_multi_rgba8, render_image_normals, render_image_rgba8, render_rays, render_rays_device, save_pam,
                  clip_rays, clip_rays_device, dilate_occupancy, dilate_occupancy_device, render_rays_clipped, render_rays_clipped_device,
                  save_pfm, save_ply, save_ppm, unpack_occupancy, point_cloud, point_cloud_device, render_image_points, save_point_cloud_ply)
from .distributed import band_of_rank, partition_for, render_image_distributed  # noqa: F401

# FLOPs per evaluated point.  FULL is what the f32 kernels EXECUTE: they run the activation-free bottleneck folded into the viewdirs
# layer (W' = W_b . W_v[0:256], formed once per loaded network), 2 x 256 x 256 FLOPs fewer than the reference's graph, whose figure
# stays beside it.  Rooflines are priced on executed work.  The 16-bit arithmetics (bf16, bf16x3, f16x2) still execute the unfolded
# head: their full evaluations are priced 11 % low until they fold as well.
FLOP_PER_POINT_FULL = 1_055_744
FLOP_PER_POINT_FULL_REFERENCE_GRAPH = 1_186_816
FLOP_PER_POINT_SIGMA = 982_528


def flop_per_ray(n_coarse, n_fine, coarse_only=False):
    """Executed FLOPs per ray of the f32 path (minus the folded bottleneck): coarse sigma-only + fine full on the merged samples."""
    if coarse_only:
        return n_coarse * FLOP_PER_POINT_FULL
    return n_coarse * FLOP_PER_POINT_SIGMA + (n_coarse + n_fine) * FLOP_PER_POINT_FULL
