"""The NOVEL_PE deformation-map builder alone (csrc/novel_pe_map.hip), through the C ABI (diner_pack_novel_pe_map): out [T, C] =
F [T, C] . W^T with W [C, C] row-major, an exact fp32 GEMM of 64-texel tiles, 32-column output tiles dealt to eight waves and K in
512-column pieces.  A ``DinerScene`` of SB = 1, NV = 1, h = 1, w = T gives any texel count T, which the renderer's square latents never
do (24 x 24 = 576 = 9 x 64):
    T = 1, 63, 65, 130   a tail tile: the ``t < T`` store guard and the ``T - 1`` load clamp (one tile; two; three)
    T = 64               no tail
    C = 8, 40, 264       dead lanes (C % 32 != 0), one and two trips over the column tiles
    C = 512              a single full piece, two trips
    C = 520, 776, 1016   the second K piece (8, 264, 504 columns), re-staged on every trip, with and without dead lanes
For every (T, C), twice (a permutation matrix W; random W):
  * sentinels: the output sits inside a larger buffer, it and a guard of 64 C floats on either side preset to a NaN of a known bit
    pattern; afterwards every output is finite and every guard word still holds the pattern;
  * W a seeded permutation matrix, F without zeros: out[t, n] == F[t, perm[n]] bit for bit (every product is F x 1 or F x 0 = +-0), which
    pins every row and column index of the staging, the MFMA operand layout and the store, in both pieces and in the tail tile;
  * random W, the rows of F scaled by seeded magnitudes from 1e-3 to 1e3: |out - F W^T| <= (C + 2) 2^-24 (|F| |W|^T) per element against
    the float64 product: the forward bound of a C-term float32 dot product (tests/gemm_refs.py holds the training GEMMs to the same),
    which holds for any summation order.
tests/test_gpu_novel_pe_point.py::test_identity_deformation_is_the_novel_kernel_bit_for_bit covers W = I on the renderer's route."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TS = (1, 63, 64, 65, 130)
CS = (8, 40, 264, 512, 520, 776, 1016)
SENTINEL = 0x7FC0BEEF          # a quiet NaN with a payload no arithmetic produces
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def build_map(F, W, dev):
    """diner_pack_novel_pe_map on F [T,C], W [C,C] (float32 numpy) -> (out [T,C] numpy, the guard words before, the guard words after)"""
    from diner_amd import _lib
    T, Cc = F.shape
    guard = 64 * Cc
    lat, w = torch.from_numpy(F).to(dev), torch.from_numpy(W).to(dev)
    buf = torch.full((guard + T * Cc + guard,), SENTINEL, dtype=torch.int32, device=dev)
    out = buf[guard:guard + T * Cc]
    sc = _lib.DinerScene()
    sc.SB, sc.NV, sc.h, sc.w, sc.C = 1, 1, 1, T, Cc
    sc.latent = lat.data_ptr()
    L = _lib.lib()
    assert L.diner_novel_pe_map_floats(C.byref(sc)) == T * Cc
    _lib.check(L.diner_pack_novel_pe_map(C.byref(sc), C.c_void_p(w.data_ptr()), C.c_void_p(out.data_ptr()),
                                         C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "diner_pack_novel_pe_map")
    torch.cuda.synchronize(dev)
    host = buf.cpu().numpy()
    return host[guard:guard + T * Cc].view(np.float32).reshape(T, Cc), host[:guard], host[guard + T * Cc:]


def check_sentinels(out, before, after):
    assert np.isfinite(out).all(), f"{int((~np.isfinite(out)).sum())} outputs were never written (or are not finite)"
    assert (before == SENTINEL).all() and (after == SENTINEL).all(), "a store left the output"


@pytest.mark.parametrize("Cc", CS)
@pytest.mark.parametrize("T", TS)
def test_permutation_matrix_moves_every_element_bit_for_bit(T, Cc, dev):
    rs = np.random.RandomState(7000 + 10 * Cc + T)
    F = (rs.uniform(0.5, 2.0, (T, Cc)) * rs.choice([-1.0, 1.0], (T, Cc))).astype(np.float32)
    perm = rs.permutation(Cc)
    W = np.zeros((Cc, Cc), np.float32)
    W[np.arange(Cc), perm] = 1.0
    assert (F != 0).all() and not np.array_equal(perm, np.arange(Cc))
    out, before, after = build_map(F, W, dev)
    check_sentinels(out, before, after)
    want = F[:, perm]
    bad = np.argwhere(out.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{len(bad)} of {out.size} differ, the first at (t, n) = {tuple(bad[0])}: {out[tuple(bad[0])]} != {want[tuple(bad[0])]}"


_worst = {}


@pytest.mark.parametrize("Cc", CS)
@pytest.mark.parametrize("T", TS)
def test_random_product_meets_the_dot_product_bound(T, Cc, dev):
    rs = np.random.RandomState(9000 + 10 * Cc + T)
    F = (rs.standard_normal((T, Cc)) * 10.0 ** rs.uniform(-3, 3, (T, 1))).astype(np.float32)
    W = (rs.uniform(-1, 1, (Cc, Cc)) / np.sqrt(Cc)).astype(np.float32)
    out, before, after = build_map(F, W, dev)
    check_sentinels(out, before, after)
    F64, W64 = F.astype(np.float64), W.astype(np.float64)
    want, absr = F64 @ W64.T, np.abs(F64) @ np.abs(W64).T
    bound = (Cc + 2) * U * absr
    err = np.abs(out.astype(np.float64) - want)
    ratio = float((err / bound).max())
    _worst[T, Cc] = ratio
    print(f"T={T} C={Cc}: max error / bound {ratio:.4f}; in units of 2^-24 (|F| |W|^T): {float((err / (U * absr)).max()):.2f}; "
          f"largest so far {max(_worst.values()):.4f}")
    assert (err <= bound).all(), f"error / bound up to {ratio:.3f}"
