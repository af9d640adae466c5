"""Drop-in for the reference's `diff_lidargs_surfel_rasterization` package (BASELINE config 5).

Same public surface as R2/diff_lidargs_surfel_rasterization/__init__.py: `GaussianRasterizationSettings`
(14 fields, :188-202), `GaussianRasterizer` with forward / markVisible / visible_filter (:204-273) and the
functional `rasterize_gaussians` (:21-43).  forward returns (color[2,H,W], radii[P], others[7,H,W], pixels[P,1]);
gradients flow to means3D, means2D (the [P,4] densification statistics), colors_precomp, opacities, scales[P,2]
and rotations -- and, beyond the reference, to raster_settings.viewmatrix (the sensor pose) when that tensor requires grad (not together
with a precomputed transform).  A precomputed transform (`cov3Ds_precomp` = transMat_precomp [P,9]) is honoured as the reference honours it --
given NEXT TO scales / rotations through the functional `rasterize_gaussians`, it replaces the rows the blends use, and receives
dL_dtransMat; spherical harmonics are not part of the LiDAR path (rejected natively).
"""
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _C


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    bg: torch.Tensor
    scale_modifier: float
    depth_threshold: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    beam_inclinations: torch.Tensor
    lidar_far: int
    lidar_near: int
    debug: bool


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
        rs = raster_settings
        num_rendered, color, others, radii, pixels, geom, binning, img = _C.rasterize_gaussians(
            rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp, rs.viewmatrix,
            rs.projmatrix, rs.beam_inclinations, rs.image_height, rs.image_width, sh, rs.sh_degree, rs.campos, rs.prefiltered,
            rs.lidar_far, rs.lidar_near, rs.debug)
        ctx.raster_settings = rs
        ctx.num_rendered = num_rendered
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geom, binning, img)
        ctx.mark_non_differentiable(radii, pixels)
        ctx.set_materialize_grads(False)      # no zero tensors for radii / pixels; backward fills in a missing image gradient
        return color, radii, others, pixels

    @staticmethod
    def backward(ctx, grad_out_color, grad_radii, grad_others, grad_pix):
        rs = ctx.raster_settings
        colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geom, binning, img = ctx.saved_tensors
        plane = lambda g, c: g if g is not None else torch.zeros((c, rs.image_height, rs.image_width), dtype=torch.float32, device=means3D.device)
        grad_out_color, grad_others = plane(grad_out_color, 2), plane(grad_others, 7)
        (grad_means2D, grad_colors, grad_opacities, grad_means3D, grad_transMat, grad_sh, grad_scales, grad_rotations,
         _depth) = _C.rasterize_gaussians_backward(
            rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp, rs.viewmatrix,
            rs.projmatrix, rs.beam_inclinations, grad_out_color, grad_others, sh, rs.sh_degree, rs.campos, geom,
            ctx.num_rendered, binning, img, rs.debug, want_intermediates=bool(cov3Ds_precomp.numel()))
        return (grad_means3D, grad_means2D, grad_sh if sh.numel() else None, grad_colors, grad_opacities, grad_scales,
                grad_rotations, grad_transMat if cov3Ds_precomp.numel() else None, None)


class _RasterizeGaussiansPose(torch.autograd.Function):
    """The node of a frame whose `raster_settings.viewmatrix` requires grad (no reference counterpart): that tensor is one more input, in
    front of `_RasterizeGaussians`' nine, and the backward asks the library for its gradient as well (lgsfpose_backward_view).  A node of
    its own, so that the node above -- every other frame's -- stays what it was, line for line."""

    @staticmethod
    def forward(ctx, viewmatrix, *inputs):
        _C.refuse_pose_with_transmat(inputs[7])                         # here, not first in backward
        return _RasterizeGaussians.forward(ctx, *inputs)                # (raster_settings.viewmatrix is this tensor)

    @staticmethod
    def backward(ctx, grad_out_color, grad_radii, grad_others, grad_pix):
        rs = ctx.raster_settings
        colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geom, binning, img = ctx.saved_tensors
        plane = lambda g, c: g if g is not None else torch.zeros((c, rs.image_height, rs.image_width), dtype=torch.float32, device=means3D.device)
        (grad_means2D, grad_colors, grad_opacities, grad_means3D, _grad_transMat, grad_sh, grad_scales, grad_rotations, _depth,
         grad_viewmatrix) = _C.rasterize_gaussians_backward(
            rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp, rs.viewmatrix,
            rs.projmatrix, rs.beam_inclinations, plane(grad_out_color, 2), plane(grad_others, 7), sh, rs.sh_degree, rs.campos, geom,
            ctx.num_rendered, binning, img, rs.debug, want_intermediates=False, want_viewmatrix_grad=True)
        # float32 [4, 4] in the layout of raster_settings.viewmatrix, then the nine slots of the node above
        return (grad_viewmatrix.reshape(rs.viewmatrix.shape), grad_means3D, grad_means2D, grad_sh if sh.numel() else None, grad_colors,
                grad_opacities, grad_scales, grad_rotations, None, None)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
    # The sensor pose is differentiable on request: a viewmatrix that requires grad becomes one more tensor input of the node and
    # receives dL/dviewmatrix (culling, the beam model's pixel decisions, pruning and binning are not differentiated).  Otherwise the
    # node is called exactly as before.
    if raster_settings.viewmatrix.requires_grad and torch.is_grad_enabled():
        return _RasterizeGaussiansPose.apply(raster_settings.viewmatrix, means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                             cov3Ds_precomp, raster_settings)
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                     raster_settings)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        with torch.no_grad():
            rs = self.raster_settings
            return _C.mark_visible(positions, rs.viewmatrix, rs.projmatrix)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        empty = torch.empty(0, dtype=torch.float32, device=means3D.device)
        return rasterize_gaussians(
            means3D, means2D, empty if shs is None else shs, empty if colors_precomp is None else colors_precomp, opacities,
            empty if scales is None else scales, empty if rotations is None else rotations,
            empty if cov3D_precomp is None else cov3D_precomp, self.raster_settings)

    def visible_filter(self, means3D, scales=None, rotations=None, cov3D_precomp=None):
        rs = self.raster_settings
        empty = torch.empty(0, dtype=torch.float32, device=means3D.device)
        with torch.no_grad():
            return _C.rasterize_aussians_filter(
                means3D, empty if scales is None else scales, empty if rotations is None else rotations, rs.scale_modifier,
                empty if cov3D_precomp is None else cov3D_precomp, rs.viewmatrix, rs.projmatrix, rs.beam_inclinations,
                rs.image_height, rs.image_width, rs.prefiltered, rs.lidar_far, rs.lidar_near, rs.debug)
