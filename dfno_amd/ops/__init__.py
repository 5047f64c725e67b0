from .pointwise import linear_nd, add_gelu, gelu, linear_res_gelu
from .spectral import spectral_conv
from .projhead import proj_head, proj_head_supported
from .fft import rfft_trunc, fft_trunc, pad_ifft, pad_irfft
from .lifthead import lift_head, lift_head_supported, lift_head_wide_range
from .epilogue import (block_epilogue, irfft_linear_res_gelu,
                       fused_epilogue_enabled, fused_epilogue_ok)
