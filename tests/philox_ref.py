"""Host restatement (numpy, no GPU) of the noise the sampler draws in its kernels when none is injected -- the stream contract of
DESIGN.md section 2 / INTEGRATION.md, and the only place the test suite encodes it.  tests/test_philox_ref_host.py proves the
restatement (known answers, distinct counters, statistics, rejection of wrong variants); tests/test_gpu_philox.py holds the kernels
to it.

Philox4x32-10, key = (seed_lo, seed_hi) of the call seed ``call_seed(renderer.seed, n)`` of the renderer's n-th call (n = 1, 2, ..),
counter (x, y, gray_lo, gray_hi) with gray = sb * NR + ray, the row of the dense tensors:

    stream       y   x                               word            value
    candidates   0   (j & 63) | ((j >> 8) << 6)      (j >> 6) & 3    u01            -> u_coarse[gray, j]
    gaussian     1   slot i                          .x, .y          Box-Muller     -> n_gauss[gray, i]
    fill-up      2   rank (i-th empty slot)          .x              u01            -> u_fill[gray, i]

u01(w) = (w >> 8) * 2^-24 is exact in float32, so ``u_coarse`` and ``u_fill`` are exact; the gaussian is
sqrt(-2 ln(1 - u1)) cos(2 pi u2): ``n_gauss64`` in float64, ``n_gauss32`` in numpy float32 with the kernel's literals.

Every restatement takes ``defect=<name>`` (DEFECTS): a deliberately wrong variant, which the CPU tests show the comparisons reject.
"""
from __future__ import annotations

import numpy as np

from tests import stage_refs as sr

F32 = np.float32
U64 = np.uint64
MASK32 = U64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = U64(0xD2511F53), U64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = U64(0x9E3779B9), U64(0xBB67AE85)
SEED_MUL = 0x9E3779B97F4A7C15
STREAM_CANDIDATES, STREAM_GAUSS, STREAM_FILL = 0, 1, 2
DEFECTS = ("always_x", "shift6", "ignore_stream", "ignore_key_hi", "rank_as_slot")


def philox4x32(ctr, key):
    """Philox4x32-10.  ctr: four arrays (or ints) that broadcast, key: two; 32-bit words held in uint64.  -> four uint32 arrays"""
    x, y, z, w = np.broadcast_arrays(*[np.asarray(c, dtype=U64) & MASK32 for c in ctr])
    k0, k1 = [np.asarray(k, dtype=U64) & MASK32 for k in key]
    for _ in range(10):
        p0, p1 = PHILOX_M0 * x, PHILOX_M1 * z              # 32 x 32 -> 64 bits: no overflow in uint64
        x, y, z, w = (p1 >> U64(32)) ^ y ^ k0, p1 & MASK32, (p0 >> U64(32)) ^ w ^ k1, p0 & MASK32
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return tuple(a.astype(np.uint32) for a in (x, y, z, w))


def u01(word):
    """[0, 1) from the upper 24 bits: exact in float32"""
    return (np.asarray(word, dtype=np.uint32) >> np.uint32(8)).astype(F32) * F32(1.0 / 16777216.0)


def call_seed(seed, calls):
    """the seed of a renderer's ``calls``-th call (1 = the first after ``renderer.seed, renderer._calls = seed, 0``)"""
    return (int(seed) * SEED_MUL + int(calls)) & 0xFFFFFFFFFFFFFFFF


def _key(seed, defect):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, 0 if defect == "ignore_key_hi" else seed >> 32


def _draw(seed, x, stream, gray, defect):
    """the four words of counter (x, stream, gray_lo, gray_hi): x [n_cols] or [n_rays, n_cols], gray [n_rays] -> 4 x [n_rays, n_cols]"""
    gray = np.asarray(gray, dtype=U64)[:, None]
    x = np.asarray(x, dtype=U64)
    x = x[None, :] if x.ndim == 1 else x
    y = 0 if defect == "ignore_stream" else stream
    return philox4x32((x, y, gray & MASK32, gray >> U64(32)), _key(seed, defect))


def _rows(n_rays, gray):
    return np.arange(n_rays, dtype=np.int64) if gray is None else np.asarray(gray, dtype=np.int64)


def candidate_counter(j, defect=None):
    """candidate j -> (counter word x, component 0..3): one Philox call serves the 4 candidates lane + 64 (4 g .. 4 g + 3) of a lane"""
    j = np.asarray(j, dtype=np.int64)
    x = (j & 63) | ((j >> (6 if defect == "shift6" else 8)) << 6)
    comp = np.zeros_like(j) if defect == "always_x" else (j >> 6) & 3
    return x, comp


def u_coarse(seed, n_rays, NC, defect=None, gray=None):
    """[n_rays, NC] float32: row = gray (default 0 .. n_rays - 1), column = candidate j"""
    x, comp = candidate_counter(np.arange(NC), defect)
    words = np.stack(_draw(seed, x, STREAM_CANDIDATES, _rows(n_rays, gray), defect), 0)            # [4, n_rays, NC]
    return u01(np.take_along_axis(words, np.broadcast_to(comp[None, None, :], (1,) + words.shape[1:]), 0)[0])


def u_fill(seed, n_rays, K, defect=None, gray=None, z_dg=None):
    """[n_rays, K] float32: column i = the i-th empty slot (rank i) of the ray.  ``defect='rank_as_slot'`` needs the samples before the
    fill-up, ``z_dg`` [n_rays, K]: the i-th empty slot then draws at its slot index instead of its rank"""
    x = np.arange(K, dtype=np.int64)
    if defect == "rank_as_slot":
        z = np.asarray(z_dg).reshape(n_rays, K)
        x = np.broadcast_to(x, (n_rays, K)).copy()
        for r in range(n_rays):
            slots = np.nonzero(z[r] == 0)[0]
            x[r, :slots.size] = slots
    return u01(_draw(seed, x, STREAM_FILL, _rows(n_rays, gray), defect)[0])


def gauss_uniforms(seed, n_rays, G, defect=None, gray=None):
    """(u1, u2), each [n_rays, G] float32: words .x and .y of gaussian slot i"""
    w = _draw(seed, np.arange(G, dtype=np.int64), STREAM_GAUSS, _rows(n_rays, gray), defect)
    return u01(w[0]), u01(w[1])


def n_gauss64(seed, n_rays, G, defect=None, gray=None):
    """Box-Muller in float64 on the (exact) uniforms: [n_rays, G] float64"""
    u1, u2 = [u.astype(np.float64) for u in gauss_uniforms(seed, n_rays, G, defect, gray)]
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)


def n_gauss32(seed, n_rays, G, defect=None, gray=None):
    """the kernel's expression, every operation in numpy float32 with the kernel's literal constants: [n_rays, G] float32"""
    u1, u2 = gauss_uniforms(seed, n_rays, G, defect, gray)
    return (np.sqrt(F32(-2.0) * np.log(F32(1.0) - u1)) * np.cos(F32(6.283185307179586) * u2)).astype(F32)


def noise(seed, SB, NR, NC, K, G, defect=None, z_dg=None):
    """the dense (u_coarse [SB,NR,NC], n_gauss [SB,NR,G] = n_gauss64 rounded to float32, u_fill [SB,NR,K]) of one call"""
    n = SB * NR
    return (u_coarse(seed, n, NC, defect).reshape(SB, NR, NC), n_gauss64(seed, n, G, defect).astype(F32).reshape(SB, NR, G),
            u_fill(seed, n, K, defect, z_dg=z_dg).reshape(SB, NR, K))


def delta_n(seed, n_rays, G):
    """-> (MARGIN x max |n_gauss32 - n_gauss64| over these draws, that maximum): how far a float32 evaluation of the gaussian may
    lie from the float64 one, per unit of the ray's standard deviation.  From the reference alone."""
    err = float(np.abs(n_gauss32(seed, n_rays, G).astype(np.float64) - n_gauss64(seed, n_rays, G)).max(initial=0.0))
    return sr.MARGIN * err, err


# ------------------------------------------------------------------------------------------------
# comparisons (the GPU tests' and, on the oracle's CPU stages, the rejection tests')
# ------------------------------------------------------------------------------------------------
def compare_bits(got, want, what):
    """float32 arrays bit for bit -> findings"""
    a, b = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    if a.shape != b.shape:
        return [f"{what}: shape {a.shape} != {b.shape}"]
    d = a.view(np.uint32) != b.view(np.uint32)
    if d.any():
        rows = np.nonzero(d.reshape(-1, a.shape[-1]).any(-1))[0]
        return [f"{what}: {int(d.sum())} of {d.size} values differ, on {rows.size} rays (first {rows[:5].tolist()})"]
    return []


def gauss_std(L, z_cand, K, G):
    """per ray the standard deviation the gaussian slots are scaled by: float64 select_from_likelihood with n = 1 minus n = 0 -> [NR]"""
    one, _ = sr.select_rows(L, z_cand, K, G, np.ones((L.shape[0], G)))
    zero, _ = sr.select_rows(L, z_cand, K, G, np.zeros((L.shape[0], G)))
    return (one - zero)[:, K - G] if G > 0 else np.zeros(L.shape[0])


def compare_gauss(got, want, gstd, dn, what, base=0.0):
    """|got - want| <= base + dn * gstd[ray] + FLOOR_GAUSS on [NR, n] arrays (NaN fails) -> (findings, max error, max of the bound)"""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    tol = base + dn * np.asarray(gstd, np.float64)[:, None] + sr.FLOOR_GAUSS
    err = float(np.nanmax(d, initial=0.0)) if np.isfinite(d).all() else float("inf")
    bad = [] if (d <= tol).all() else [f"{what}: max error {err:.3e}, worst excess over its bound {float(np.nanmax(d - tol)):.3e}"]
    return bad, err, float(tol.max(initial=0.0))


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
class PhiloxCase:
    """A stage_refs.SamplerCase whose dense noise is the restatement's for the call seed of (seed, calls)"""

    def __init__(self, NC, K, G, SB, seed, calls):
        self.base = sr.SamplerCase(NC, K, G, SB=SB)
        self.NC, self.K, self.G, self.SB, self.seed, self.calls = NC, K, G, SB, seed, calls
        self.call_seed = call_seed(seed, calls)
        self.id = f"NC{NC}-K{K}-G{G}-SB{SB}-seed{seed}-call{calls}"

    def build(self):
        """-> the SamplerCase with u_coarse / n_gauss / u_fill restated and its oracle expectations computed (once)"""
        c = self.base
        if not hasattr(self, "dn"):
            c.build()
            NR = c.rays.shape[1]
            c.u_coarse, c.n_gauss, c.u_fill = noise(self.call_seed, self.SB, NR, self.NC, self.K, self.G)
            self.dn, self.n32_err = delta_n(self.call_seed, self.SB * NR, self.G)
            c.oracle()
        return c


# (seed, calls) -> call seed: (0, 1) -> 1 and (0, 7) -> 7 (< 2^32: key word 1 is zero); (1, 1) -> 0x9E3779B97F4A7C16 and
# (3, 2) -> 0xDAA66D2C7DDF7441 (>= 2^63: negative as the torch op's int64); (2, 5) -> 0x3C6EF372FE94F82F (both key words set, < 2^63)
SEEDS = ((0, 1), (1, 1), (3, 2), (2, 5), (0, 7))
# NC: all four candidates-per-lane variants, not multiples of 64 / 256, j >> 8 > 0.  (K, G): K and G beyond 64 (the 64-slot loops run more
# than once), G = 0, G = K.  K <= NC.  Paired, not the full product; every NC, every (K, G), both SB and every seed occur.
_SHAPES = [(63, 16, 5, 1), (63, 12, 0, 2), (200, 40, 15, 2), (200, 128, 48, 1), (200, 12, 12, 1), (1024, 256, 96, 1), (1024, 12, 0, 1),
           (2048, 128, 48, 2), (2048, 16, 5, 1), (4096, 256, 96, 2), (4096, 40, 15, 1), (4096, 12, 12, 1)]
PHILOX_CASES = [PhiloxCase(*s, *SEEDS[i % len(SEEDS)]) for i, s in enumerate(_SHAPES)]
