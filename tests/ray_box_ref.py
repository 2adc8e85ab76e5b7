"""float64 numpy restatement of diner_amd/csrc/ray_box.hip (glue.ray_box, glue.box_rays, glue.frame_from_hits), written from the
formulas of include/diner_hip.h, not from the kernels:

* ``gen_rays_ref``        gen_rays' rays: pixel centres, unit directions, OpenCV convention (reference src/util/cam_geometry.py:36-79)
* ``box_near_far_ref``    the six face planes, the signed t0 <= t1 of the faces that count, the clamp to [z_near, z_far], the hit test; also
                          the *ambiguous set* of the rays
* ``select_ref``          the ordered compaction: idx, slot, count
* ``frame_from_hits_ref`` the gather through slot
* ``compare``             the comparison every test makes between a result and an expectation, outside the ambiguous set

The ambiguous set: pixels for which some face-plane intersection lies within ``AMBIGUOUS`` = 1e-4 of another axis' face (moved out by
eps), or whose clamped ``far - near`` is below 1e-4 in magnitude.  There a rounding of the inputs decides the mask; every mask comparison
is made outside it, and it may hold at most ``CAP`` = 1 % of a test's pixels (a condition of the comparison, not a measurement).

``variant`` builds the deliberately wrong forms the host test must see rejected.
"""
import numpy as np

EPS = 1e-6
SMALL_DIR = 1e-5
AMBIGUOUS = 1e-4
CAP = 0.01
BOX_OFFSET = (-0.01, 0.01)
VARIANTS = ("corners", "no_offset", "one_sign_offset", "swap_near_far", "unsorted_idx")


def look_at(eye, target=(0.0, 0.0, 0.0)):
    """world->camera [4,4] float64 of a camera at ``eye`` looking at ``target``, image y along world +y as far as the view allows"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    E = np.eye(4)
    E[:3, :3] = np.stack([x, y, z])
    E[:3, 3] = -E[:3, :3] @ eye
    return E


def intrinsics(f, H, W):
    return np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])


def gen_rays_ref(E, K, H, W, variant=None):
    """origins [H,W,3], unit directions [H,W,3] in float64 of one camera E [4,4], K [3,3]"""
    E, K = np.asarray(E, np.float64), np.asarray(K, np.float64)
    half = 0.0 if variant == "corners" else 0.5
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64) + half, np.arange(H, dtype=np.float64) + half, indexing="xy")
    d = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], axis=-1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    R, t = E[:3, :3], E[:3, 3]
    return np.broadcast_to(-R.T @ t, d.shape).copy(), d @ R


def box_near_far_ref(o, d, bounds, z_near, z_far, box_offset=BOX_OFFSET, variant=None):
    """o, d [...,3]; bounds [2,3] -> near, far, mask, ambiguous [...] (a miss holds z_near, z_far)"""
    o, d, bounds = np.asarray(o, np.float64), np.asarray(d, np.float64), np.asarray(bounds, np.float64)
    lo, hi = box_offset
    if variant == "no_offset":
        lo = hi = 0.0
    elif variant == "one_sign_offset":
        hi = lo
    b = np.stack([bounds[0] + lo, bounds[1] + hi])
    d = np.where(np.abs(d) < SMALL_DIR, SMALL_DIR, d)
    t0 = np.full(o.shape[:-1], np.inf)
    t1 = np.full(o.shape[:-1], -np.inf)
    faces = np.zeros(o.shape[:-1], np.int64)
    amb = np.zeros(o.shape[:-1], bool)
    for side in (0, 1):
        for a in range(3):
            t = (b[side, a] - o[..., a]) / d[..., a]
            on = np.ones(o.shape[:-1], bool)
            for u in ((a + 1) % 3, (a + 2) % 3):
                p = t * d[..., u] + o[..., u]
                on &= (p >= b[0, u] - EPS) & (p <= b[1, u] + EPS)
                amb |= (np.abs(p - (b[0, u] - EPS)) < AMBIGUOUS) | (np.abs(p - (b[1, u] + EPS)) < AMBIGUOUS)
            t0 = np.where(on, np.minimum(t0, t), t0)
            t1 = np.where(on, np.maximum(t1, t), t1)
            faces += on
    n, f = np.maximum(t0, z_near), np.minimum(t1, z_far)
    with np.errstate(invalid="ignore"):
        amb |= (faces >= 1) & (np.abs(f - n) < AMBIGUOUS)
    mask = (faces >= 2) & (f > n)
    near, far = np.where(mask, n, z_near), np.where(mask, f, z_far)
    if variant == "swap_near_far":
        near, far = far, near
    return near, far, mask, amb


def select_ref(mask, variant=None):
    """mask [H,W] -> idx [H W] (the hit pixels ascending, then -1), slot [H W], count"""
    flat = np.asarray(mask, bool).reshape(-1)
    hits = np.flatnonzero(flat).astype(np.int32)
    if variant == "unsorted_idx" and hits.size > 1:
        hits = hits[::-1].copy()
    idx = np.full(flat.size, -1, np.int32)
    idx[:hits.size] = hits
    slot = np.full(flat.size, -1, np.int32)
    slot[hits] = np.arange(hits.size, dtype=np.int32)
    return idx, slot, int(hits.size)


def ray_box_ref(E, K, H, W, z_near, z_far, bounds, box_offset=BOX_OFFSET, variant=None):
    """one camera -> dict(near, far, mask, ambiguous [H,W]; idx, slot [H W]; count; o, d [H,W,3])"""
    o, d = gen_rays_ref(E, K, H, W, variant)
    near, far, mask, amb = box_near_far_ref(o, d, bounds, z_near, z_far, box_offset, variant)
    idx, slot, count = select_ref(mask, variant)
    return dict(near=near, far=far, mask=mask, ambiguous=amb, idx=idx, slot=slot, count=count, o=o, d=d)


def frame_from_hits_ref(rgb_c, depth_c, slot, H, W, white_bkgd):
    """rgb_c [B,3], depth_c [B], slot [H W] -> rgb [3,H,W], depth [1,H,W]"""
    slot = np.asarray(slot).reshape(-1)
    hit = slot >= 0
    rgb = np.full((slot.size, 3), 1.0 if white_bkgd else 0.0, np.asarray(rgb_c).dtype)
    depth = np.zeros(slot.size, np.asarray(depth_c).dtype)
    rgb[hit] = np.asarray(rgb_c)[slot[hit]]
    depth[hit] = np.asarray(depth_c)[slot[hit]]
    return rgb.reshape(H, W, 3).transpose(2, 0, 1), depth.reshape(1, H, W)


def tolerance(far):
    """near / far: 1e-6 max(1, far).  One fp32 subtraction and one division per face, <= 2 ulp (2^-23 each) of a value near 2, on rays
    that are float32 roundings of the float64 ones"""
    return 1e-6 * np.maximum(1.0, np.abs(far))


def compare(got, want, ambiguous):
    """got: near, far, mask [H,W] (+ idx, slot [H W], count when present); want: near, far, mask; ambiguous [H,W].
    -> the list of what is wrong (empty: the result passes)"""
    bad = []
    amb = np.asarray(ambiguous, bool)
    gm, wm = np.asarray(got["mask"], bool), np.asarray(want["mask"], bool)
    if amb.mean() > CAP:
        bad.append(f"the ambiguous set holds {amb.mean():.2%} of the pixels, more than {CAP:.0%}")
    if ((gm != wm) & ~amb).any():
        bad.append(f"{int(((gm != wm) & ~amb).sum())} mask mismatches outside the ambiguous set")
    both = gm & wm & ~amb
    tol = tolerance(np.asarray(want["far"], np.float64))
    for k in ("near", "far"):
        miss = np.abs(np.asarray(got[k], np.float64) - np.asarray(want[k], np.float64))
        if (miss[both] > tol[both]).any():
            bad.append(f"{k} off by up to {miss[both].max():.3e} (allowed {tol[both].min():.1e} and up)")
    if "idx" in got:
        idx, slot, count = np.asarray(got["idx"]).reshape(-1), np.asarray(got["slot"]).reshape(-1), int(got["count"])
        hits = np.flatnonzero(gm.reshape(-1))
        if count != hits.size:
            bad.append(f"count {count} != mask.sum() {hits.size}")
        elif not np.array_equal(idx[:count], hits):
            bad.append("idx[:count] is not the hit pixels in ascending order")
        else:
            inv = np.full(slot.size, -1, np.int64)
            inv[idx[:count]] = np.arange(count)
            if not np.array_equal(slot, inv):
                bad.append("slot is not the inverse of idx")
    return bad
