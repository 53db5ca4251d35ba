"""manigaussian_amd -- MI355X-native (gfx950) Gaussian-splatting hot path of ManiGaussian.

Scope: the differentiable tile rasterizer (RGB + feature channels, fwd+bwd) behind the
reference's GaussianRasterizer / GaussianRasterizationSettings API, and the deformation-field per-Gaussian
apply.  Native code: manigaussian_amd/csrc (HIP) -> libmgsplat.so, C ABI in include/mgsplat.h.
"""
from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer, rasterize_gaussians  # noqa: F401
from .views import GaussianRasterizerBatch  # noqa: F401
from .regressor import gaussian_epilogue  # noqa: F401
from .voxel import point_latent_pe  # noqa: F401
from .losses import manigaussian_losses, rendering_loss  # noqa: F401
from .photometric import l1_loss, photometric_loss, ssim  # noqa: F401
from .optim import FusedLamb  # noqa: F401
from .voxelizer import VoxelGrid, voxelize_images  # noqa: F401
from .attention import Attention, fused_attention  # noqa: F401
from .spatial_softmax import SpatialSoftmax3D, spatial_softmax3d  # noqa: F401
from .volume import Conv3DBlock, Conv3DUpsampleBlock, resample_pad  # noqa: F401
from .feedforward import GEGLU, FeedForward, PreNorm, bias_geglu, layer_norm  # noqa: F401
from .encoder import ConvBnReLU3D, InPlaceABN, MultiLayer3DEncoderShallow, batch_norm_act  # noqa: F401
from .conv3d import conv3d, conv_transpose3d  # noqa: F401
from .pointwise import pointwise_conv3d, wide_pointwise_conv3d  # noqa: F401
from .narrow import narrow_conv3d  # noqa: F401
from .dense import dense_conv3d  # noqa: F401
from .patch import patch_conv3d  # noqa: F401
from .augmentation import (Se3Augmentation, apply_se3_augmentation,  # noqa: F401
                           apply_se3_augmentation_with_camera_pose)
from . import camera  # noqa: F401
from ._state import (check_status, forward_mode, overflow_policy, set_forward_mode, set_headroom,  # noqa: F401
                     set_overflow_policy, set_safe_workspace)

__version__ = "0.1.0"
