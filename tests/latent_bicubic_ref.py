"""A numpy restatement of the encoder's tail with upsample_interp="bicubic" -- F.interpolate(mode="bicubic", align_corners=True) per level
and cat (reference src/models/image_encoder.py:262-272; ATen's upsample_bicubic2d) -- as one dense matrix per axis, and the cases, inputs
and bounds that tests/test_latent_assemble_bicubic_host.py (which proves the restatement against CPU torch) and
tests/test_gpu_latent_assemble_bicubic.py (which holds the kernels to it) share.

Per axis:  scale = (in - 1) / (out - 1) in fp32 (0 when out == 1);  src = scale * dst in fp32;  i = min((int)src, in - 1);  t = src - i;
taps i - 1 .. i + 2, each clamped to [0, in - 1];  A = -0.75;
    w0 = ((A (t + 1) - 5 A) (t + 1) + 8 A) (t + 1) - 4 A        w1 = ((A + 2) t - (A + 3)) t t + 1
    w3 = ((A (2 - t) - 5 A) (2 - t) + 8 A) (2 - t) - 4 A        w2 = ((A + 2) (1 - t) - (A + 3)) (1 - t) (1 - t) + 1
The taps are placed in fp32 (as ATen and the kernels place them) whatever the dtype of the coefficients.  With dtype=float64 the matrices
are the oracle.  ``factored=True`` evaluates the same cubics the way the kernels do, w0 = A t (1 - t)^2 and
w1 = (1 - t) (1 + t - (A + 2) t^2) (w3, w2: the same of 1 - t): with dtype=float32 these are the kernels' own coefficients, operation by
operation.  (In fp32 the Horner forms above leave up to 12 * 2^-24 absolute on coefficients as small as 0.02 -- intermediates of
magnitude 3..6 -- and the adjoint built on them misses the backward bound below by a factor of up to 2.5 on the cases "downsample" and
"one_axis", where a coarse texel has only a few fine pixels on it; the factored forms stay below a tenth of it.)"""
import numpy as np

ULP = 2.0 ** -23

# name -> (SB, NV, [(C_l, h_l, w_l), ...]); the output takes the first level's size
CASES = {
    "ragged_five_levels": (2, 3, [(8, 11, 13), (8, 6, 7), (16, 3, 4), (24, 2, 2), (8, 1, 1)]),   # 143 pixels: ragged tiles; in = 1, 2, 3; C = 64
    "out_1x1": (1, 2, [(8, 1, 1), (8, 3, 3)]),                                                    # scale 0
    "resnet": (1, 2, [(64, 20, 20), (64, 10, 10), (128, 5, 5), (256, 3, 3)]),
    "c1024": (1, 1, [(256, 6, 6), (256, 3, 3), (256, 2, 2), (128, 1, 1), (128, 4, 5)]),           # C at its limit; a ragged last LDS piece
    "big_ratio": (1, 1, [(8, 20, 20), (8, 2, 2)]),                                                # largest support per texel; borders only
    "one_axis": (1, 2, [(8, 6, 10), (8, 6, 5), (8, 3, 10)]),                                      # in == out on one axis
    "downsample": (1, 3, [(8, 5, 6), (16, 7, 9), (8, 5, 9)]),                                     # levels larger than the output
}

# Forward bound against torch's CPU fp32, c_f * 2^-23 * max|level| per element.  One output value is sum_i wy_i * (sum_j wx_j * v_ij).
# Roundings on the way to it in torch's expression: src (1) and the longest coefficient (w0 / w3 in Horner form: 7 operations) per axis
# = 8 + 8; the inner sum, 4 products + 3 additions = 7; the outer sum, again 7: 30 (the kernels' factored coefficients take 6 operations:
# 28).  Each rounding is at most half an ulp of an intermediate whose magnitude the absolute weight sum bounds,
# (sum_i |wy_i|) (sum_j |wx_j|) max|level| <= 1.375^2 max|level| (sum |w| peaks at t = 1/2: 2 * 0.09375 + 2 * 0.59375 = 1.375),
# so the two results lie within (30 + 28) / 2 < 30 such ulps of each other.
C_F = 30 * 1.375 ** 2            # 56.71875, below the cap of 64
# Backward bound against the float64 restatement, (n + c_b) * 2^-23 * A per element: n terms summed in any order + the roundings of one
# term's weight: the longest factored coefficient (w1: 1 - t, 1 + t, (A + 2) t, * t, the difference, the product = 6) per axis, wy * wx (1),
# the product with d_out (1) = 14, and one addition per axis where two clamped taps coincide (a level of 2 or 3 texels along an axis; where
# all four coincide, in == 1, every fine pixel is on the texel and n is the whole output).
C_B = 6 + 6 + 1 + 1 + 2          # 16


def taps(n_in, n_out):
    """i [n_out] (int64) and t [n_out] (fp32), placed in fp32"""
    f = np.float32
    s = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)
    src = s * np.arange(n_out, dtype=f)
    i = np.minimum(src.astype(np.int64), n_in - 1)
    return i, src - i.astype(f)


def coefficients(t, dtype, A=-0.75, factored=False):
    """[4, n] cubic convolution coefficients of the fp32 fractions t, evaluated in ``dtype`` in the order written above"""
    t = t.astype(dtype)
    A, one, two = dtype(A), dtype(1), dtype(2)
    t1, u, u1 = t + one, one - t, two - t
    if factored:
        return np.stack(((A * t) * (u * u), u * ((one + t) - ((A + two) * t) * t), t * ((one + u) - ((A + two) * u) * u), (A * u) * (t * t)))
    five, eight, four = dtype(5) * A, dtype(8) * A, dtype(4) * A
    return np.stack((((A * t1 - five) * t1 + eight) * t1 - four,
                     ((A + two) * t - (A + dtype(3))) * t * t + one,
                     ((A + two) * u - (A + dtype(3))) * u * u + one,
                     ((A * u1 - five) * u1 + eight) * u1 - four))


def weights_1d(n_in, n_out, dtype=np.float64, A=-0.75, factored=False):
    """The dense [n_out, n_in] matrix of one axis: the coefficients of clamped taps that coincide are added (tap order ascending)."""
    i, t = taps(n_in, n_out)
    c = coefficients(t, dtype, A, factored)
    W = np.zeros((n_out, n_in), dtype=dtype)
    rows = np.arange(n_out)
    for k in range(4):
        W[rows, np.clip(i - 1 + k, 0, n_in - 1)] += c[k]
    return W


def upcat_bicubic(levels, size, dtype=np.float64, A=-0.75, factored=False):
    """levels: arrays [N, C_l, h_l, w_l] -> [N, sum C_l, *size]: Wy @ level @ Wx.T per level, then cat"""
    out = []
    for v in levels:
        Wy, Wx = weights_1d(v.shape[2], size[0], dtype, A, factored), weights_1d(v.shape[3], size[1], dtype, A, factored)
        out.append(np.einsum("yi,ncij,xj->ncyx", Wy, np.asarray(v, dtype=dtype), Wx))
    return np.concatenate(out, axis=1)


def adjoint_bicubic(d_out, specs, dtype=np.float64, absolute=False):
    """d_out [N, sum C_l, h, w] -> the levels' gradients Wy^T d Wx ([N, C_l, h_l, w_l] each); absolute: |Wy|^T |d| |Wx|"""
    h, w = d_out.shape[2:]
    d = np.asarray(d_out, dtype=dtype)
    out, off = [], 0
    for c, hl, wl in specs:
        Wy, Wx = weights_1d(hl, h, dtype), weights_1d(wl, w, dtype)
        g = d[:, off:off + c]
        if absolute:
            Wy, Wx, g = np.abs(Wy), np.abs(Wx), np.abs(g)
        out.append(np.einsum("yi,ncyx,xj->ncij", Wy, g, Wx))
        off += c
    return out


def support(n_in, n_out):
    """the largest number of fine indices with a non-zero weight on one coarse index"""
    return int((weights_1d(n_in, n_out) != 0).sum(axis=0).max())


class Ref:
    """inputs and float64 references of one case, computed once and left unchanged (torch tensors; numpy inside)"""

    def __init__(self, name):
        import torch
        self.SB, self.NV, self.specs = CASES[name]
        N = self.SB * self.NV
        g = torch.Generator().manual_seed(sorted(CASES).index(name) + 41)
        self.levels = [torch.randn((N, c, h, w), generator=g) * (1.0 + i) for i, (c, h, w) in enumerate(self.specs)]
        self.size = self.specs[0][1:]
        self.C = sum(c for c, _, _ in self.specs)
        self.d_out = torch.randn((N, self.C, *self.size), generator=g)
        # the oracle of the forward: torch's own CPU fp32 kernel [N, C, h, w]
        self.out = torch.cat([torch.nn.functional.interpolate(t, size=self.size, mode="bicubic", align_corners=True) for t in self.levels], 1)
        lv = [t.numpy() for t in self.levels]
        self.out64 = torch.from_numpy(upcat_bicubic(lv, self.size))                                     # float64 [N, C, h, w]
        self.grads = [torch.from_numpy(a) for a in adjoint_bicubic(self.d_out.numpy(), self.specs)]     # float64, Wy^T d Wx
        self.A = [torch.from_numpy(a) for a in adjoint_bicubic(self.d_out.numpy(), self.specs, absolute=True)]
        self.n = [support(h, self.size[0]) * support(w, self.size[1]) for _, h, w in self.specs]

    def resampled(self, spec):
        """a level that is resampled and has more than one texel: where a wrong interpolation shows"""
        _, h, w = spec
        return (h, w) != tuple(self.size) and h * w > 1


_refs = {}


def ref(name):
    if name not in _refs:
        _refs[name] = Ref(name)
    return _refs[name]
