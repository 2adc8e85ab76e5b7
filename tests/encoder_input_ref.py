"""Torch restatement of conv1's input (diner_encoder_input, include/diner_hip.h) and of its adjoint to the images, on the CPU: the
reference's Normalize + ReplicationPad2d + PositionalEncoding(padding_pe, freq_factor=pi, d_in=2) of the padding (reference
src/models/pixelnerf.py:44, src/models/image_encoder.py:222-232, src/models/positional_encoding.py:14-53), written from the header's
formulas with explicit indices, not with the reference's operators.  fp32 by default; ``dtype=torch.float64`` evaluates the same
formulas in double from the same fp32 constants and coordinates (the oracle of the GPU tests).

``variant`` builds a deliberately broken form (the host test shows that the comparison rejects each of them)."""
import math

import torch

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
VARIANTS = ("swap_xy", "interior_kept", "swap_phases", "clamp_short")


def pe_channels(pad, F):
    return 2 * (1 + 2 * F) if F >= 0 and pad > 0 else 0


def tol_pe(F):
    """2^-21 (f_max + 2), f_max = pi 2^(F-1) (0 for F <= 0): coordinate rounding <= 2^-23 scaled by f_max, one ulp of an argument
    <= f_max + pi/2 (FMA against multiply-add), 5e-7 per sine implementation, with a margin of two"""
    f_max = math.pi * 2.0 ** (F - 1) if F > 0 else 0.0
    return 2.0 ** -21 * (f_max + 2.0)


def _const(v, dtype):
    """the three channel constants as the kernel receives them: fp32 values, then widened"""
    return torch.as_tensor([float(x) for x in (v.reshape(-1).tolist() if isinstance(v, torch.Tensor) else v)],
                           dtype=torch.float32).to(dtype)


def _clamped(n, size, pad, short=0):
    """source index of every padded index; short = 1: the upper clamp one pixel short (a broken variant)"""
    return (torch.arange(n) - pad).clamp(0, max(size - 1 - short, 0))


def encoder_input_ref(images, pad, F, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype=torch.float32, xs=None, ys=None, variant=None):
    """images [N,3,H,W] -> [N, 3 + Cpe, H + 2 pad, W + 2 pad].  xs [Wp] / ys [Hp]: the pixel coordinates (default: torch.linspace in fp32)"""
    assert variant is None or variant in VARIANTS
    N, _, H, W = images.shape
    Hp, Wp, Cpe = H + 2 * pad, W + 2 * pad, pe_channels(pad, F)
    x = images.to(dtype)
    short = 1 if variant == "clamp_short" else 0
    iy, ix = _clamped(Hp, H, pad, short), _clamped(Wp, W, pad, short)
    out = torch.zeros((N, 3 + Cpe, Hp, Wp), dtype=dtype)
    out[:, :3] = (x[:, :, iy][:, :, :, ix] - _const(mean, dtype).view(1, 3, 1, 1)) / _const(std, dtype).view(1, 3, 1, 1)
    if Cpe == 0:
        return out
    xs = (torch.linspace(-1, 1, Wp) if xs is None else xs.detach().cpu().float()).to(dtype)
    ys = (torch.linspace(-1, 1, Hp) if ys is None else ys.detach().cpu().float()).to(dtype)
    v = [xs.view(1, Wp).expand(Hp, Wp), ys.view(Hp, 1).expand(Hp, Wp)]
    if variant == "swap_xy":
        v = [ys.view(Hp, 1).expand(Hp, Wp), xs.view(1, Wp).expand(Hp, Wp)]
    pi32, half_pi32 = torch.tensor(math.pi, dtype=torch.float32).to(dtype), torch.tensor(math.pi * 0.5, dtype=torch.float32).to(dtype)
    pe = torch.zeros((Cpe, Hp, Wp), dtype=dtype)
    pe[0], pe[1] = v[0], v[1]
    for j in range(2 * F):
        odd = (j % 2 == 1) != (variant == "swap_phases")
        phi = half_pi32 if odd else torch.zeros((), dtype=dtype)
        f = pi32 * 2.0 ** (j // 2)
        for i in range(2):
            pe[2 + 2 * j + i] = torch.sin(phi + v[i] * f)
    if variant != "interior_kept":
        pe[:, pad:Hp - pad, pad:Wp - pad] = 0
    out[:, 3:] = pe
    return out


def encoder_input_adjoint_ref(d_out, pad, F, std=IMAGENET_STD, dtype=torch.float64):
    """d_out [N, 3 + Cpe, Hp, Wp] -> (d_images [N,3,H,W], abs_sum [N,3,H,W], n_terms [H,W]): every image pixel sums d_out over the padded
    pixels whose clamp lands on it, rows outside, columns inside, then divides by std; abs_sum = the same sum of |d_out| / std and n_terms
    its number of terms (the summation bound of the GPU test)."""
    N, Ct, Hp, Wp = d_out.shape
    H, W = Hp - 2 * pad, Wp - 2 * pad
    assert Ct == 3 + pe_channels(pad, F) and H >= 1 and W >= 1
    g = d_out[:, :3].to(dtype)
    iy, ix = _clamped(Hp, H, pad), _clamped(Wp, W, pad)

    def gather(t):
        rows = torch.zeros((N, 3, H, Wp), dtype=dtype).index_add_(2, iy, t)
        return torch.zeros((N, 3, H, W), dtype=dtype).index_add_(3, ix, rows)

    sd = _const(std, dtype).view(1, 3, 1, 1)
    ny = torch.zeros(H, dtype=torch.int64).index_add_(0, iy, torch.ones(Hp, dtype=torch.int64))
    nx = torch.zeros(W, dtype=torch.int64).index_add_(0, ix, torch.ones(Wp, dtype=torch.int64))
    return gather(g) / sd, gather(g.abs()) / sd.abs(), ny.view(H, 1) * nx.view(1, W)
