"""Golden vectors of the NOVEL point model's training path (diner_amd/training_novel.py): the UNMODIFIED reference
``src.models.novel.novel_pixelnerf.PixelNeRF`` evaluated at given points and differentiated by its own autograd on the CPU.  Runs only
where the reference source tree exists (``oracle.ref_harness``); the tests read the committed ``tests/golden/novel_train_*.npz`` only.

    python tools/gen_novel_train_golden.py            # (re)writes tests/golden/novel_train_*.npz
    python tools/gen_novel_train_golden.py --case=novel_train_b

The scheme of tools/gen_novel_point_golden.py, whose ``case_inputs``, ``input_digests`` and ``build_reference_model`` rebuild every input
from seeds, with the gradient records of tools/gen_trainshape_golden.py: the loss is ``(rgbsigma * cotangent(cfg)).sum()`` with the seeded
cotangent below (shared with the tests), and a fixture holds the config, the input digests, ``rgbsigma`` [SB,P,4], per fusion-MLP
parameter ``g_norm`` / ``g_sum`` / ``g_probe`` (``oracle.gen_golden.grad_probe_indices``), for ``encoder.latent`` the gradient's norm, max
and probes, and for ``gen_latent`` the whole gradient where it is at most 200 kB, otherwise norm, max and probes.

The relu gate of sigma must not be a coin flip: the generator reads the fusion MLP's output (a forward hook; nothing of the reference is
changed) and asserts that no point's sigma pre-activation lies within 1e-3 of 0.  A case that fails is redrawn by the seeded rule
``pseed += 1000`` -- the generator then names the first passing seed, which goes into ``CASES`` below: the table is what the tests rebuild
the inputs from.
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from tools.gen_novel_point_golden import _GEN, _SCENE, STANDARD, build_reference_model, case_inputs, input_digests  # noqa: E402

F32 = np.float32
GEN_GRAD_WHOLE_BYTES = 200_000     # gen_latent's gradient is stored whole up to this size
LATENT_PROBES = 64
SIGMA_MARGIN = 1e-3

# name: scene (NV, C = d_latent), SB scenes, model, lookup, P points per scene, seeds -- the smallest at which each thing can go wrong
CASES = {
    # (a) a tail past a 64-row run; two scenes with different general cameras accumulating into one gen_latent
    "novel_train_a": dict(scene=dict(_SCENE, NV=4, seed=170, C=64), SB=2, num_freqs=6, mlp=dict(d_hidden=128, n_blocks=3, combine_layer=2),
                          P=70, index_interp="bilinear", index_padding="border", wseed=171, pseed=172, cseed=173, **_GEN),
    # (b) one-texel footprints; zero-weight taps outside the general map; Softplus
    "novel_train_b": dict(scene=dict(_SCENE, NV=2, seed=174, C=128), SB=1, num_freqs=6,
                          mlp=dict(d_hidden=64, n_blocks=2, combine_layer=1, beta=100.0), P=33,
                          index_interp="nearest", index_padding="zeros", wseed=175, pseed=1176, cseed=177, **_GEN),
    # (c) an odd view count in the register sum; reflection padding; exactly one 64-row run
    "novel_train_c": dict(scene=dict(_SCENE, NV=3, seed=178, C=64), SB=1, num_freqs=6, mlp=dict(d_hidden=96, n_blocks=3, combine_layer=2),
                          P=64, index_interp="bilinear", index_padding="reflection", wseed=179, pseed=180, cseed=181, **_GEN),
    # (d) no mean over views (combine_layer >= n_blocks, NV = 1); 16 channel passes per wave
    "novel_train_d": dict(scene=dict(_SCENE, NV=1, seed=182, C=1024), SB=1, num_freqs=6, mlp=dict(d_hidden=64, n_blocks=2, combine_layer=1000),
                          P=5, index_interp="bilinear", index_padding="border", wseed=183, pseed=184, cseed=185, **_GEN),
    # (e) combine_layer 0: neither latent read, both latent gradients exactly 0; a single point (pseed: one whose reference sigma is above 0)
    "novel_train_e": dict(scene=dict(_SCENE, NV=3, seed=186, C=256), SB=1, num_freqs=6, mlp=dict(d_hidden=96, n_blocks=2, combine_layer=0),
                          P=1, index_interp="bilinear", index_padding="border", wseed=187, pseed=215, cseed=189, **_GEN),
    # (std) the NOVEL config's own shape (wseed: weights under which about half of the points have sigma above 0)
    "novel_train_std": dict(scene=dict(_SCENE, NV=4, seed=190, C=512), SB=1, num_freqs=6, mlp=STANDARD, P=40,
                            index_interp="bilinear", index_padding="border", wseed=247, pseed=192, cseed=193, **_GEN),
}


def cotangent(cfg):
    """the seeded cotangent [SB,P,4] of the loss (rgbsigma * cotangent).sum(), shared by the generator and the tests"""
    return np.random.RandomState(cfg["cseed"]).standard_normal((cfg["SB"], cfg["P"], 4)).astype(F32)


def latent_probe_indices(shape):
    from oracle.gen_golden import grad_probe_indices
    return grad_probe_indices(shape, n=LATENT_PROBES, seed=7)


def gen_grad_stored_whole(cfg):
    return cfg["scene"]["C"] * cfg["gen_h"] * cfg["gen_w"] * 4 <= GEN_GRAD_WHOLE_BYTES


def latent_record(prefix, g):
    """norm, max and probes of a latent's gradient"""
    g64 = g.astype(np.float64)
    return {f"{prefix}_grad_norm": np.float64(np.sqrt((g64 ** 2).sum())), f"{prefix}_grad_max": np.float64(np.abs(g64).max()),
            f"{prefix}_grad_probe": g.reshape(-1)[latent_probe_indices(g.shape)].astype(F32)}


def _evaluate(cfg):
    """the reference under autograd -> inputs, rgbsigma, sigma pre-activation, the model"""
    import torch
    torch.manual_seed(0)
    inp = case_inputs(cfg)
    nerf = build_reference_model(inp)
    enc = nerf.encoder
    enc.latent = enc.latent.clone().requires_grad_(True)
    for p in nerf.mlp_fine.parameters():
        p.requires_grad_(True)
    assert nerf.gen_latent.requires_grad
    seen = []
    hook = nerf.mlp_fine.register_forward_hook(lambda mod, args, out: seen.append(out.detach()))
    t = lambda a: torch.from_numpy(a)
    out = nerf(t(inp["xyz_in"]), t(inp["xyz_gen"]), viewdirs=t(inp["viewdirs"]))
    hook.remove()
    assert len(seen) == 1
    pre = seen[0].reshape(cfg["SB"], cfg["P"], -1)[..., 3].numpy()
    return inp, nerf, out, pre


def gen(name, cfg, out_dir):
    import torch
    from oracle.gen_golden import grad_probe_indices
    for attempt in range(50):     # the seeded re-draw of a case whose relu gate is a coin flip
        trial = dict(cfg, pseed=cfg["pseed"] + 1000 * attempt)
        inp, nerf, out, pre = _evaluate(trial)
        if np.abs(pre).min() >= SIGMA_MARGIN:
            break
    assert attempt == 0, f"{name}: a sigma pre-activation within {SIGMA_MARGIN} of 0; the first passing seed is pseed={trial['pseed']}: put it into CASES"
    assert out.shape == (cfg["SB"], cfg["P"], 4) and torch.isfinite(out).all()
    (out * torch.from_numpy(cotangent(cfg))).sum().backward()
    fixture = dict(config=json.dumps(cfg), digests=json.dumps(input_digests(inp)), rgbsigma=out.detach().numpy().astype(F32))
    enc = nerf.encoder
    lg = (enc.latent.grad if enc.latent.grad is not None else torch.zeros_like(enc.latent)).numpy()   # combine_layer 0: not used
    gg = (nerf.gen_latent.grad if nerf.gen_latent.grad is not None else torch.zeros_like(nerf.gen_latent)).numpy()
    fixture.update(latent_record("latent", lg))
    fixture.update(latent_record("gen", gg))
    if gen_grad_stored_whole(cfg):
        fixture["gen_grad"] = gg.astype(F32)
    for pname, p in nerf.mlp_fine.named_parameters():
        gnp = p.grad.numpy()
        fixture[f"g_sum/{pname}"] = np.float64(gnp.astype(np.float64).sum())
        fixture[f"g_norm/{pname}"] = np.float64(np.sqrt((gnp.astype(np.float64) ** 2).sum()))
        fixture[f"g_probe/{pname}"] = gnp.reshape(-1)[grad_probe_indices(gnp.shape)]
    np.savez_compressed(out_dir / f"{name}.npz", **fixture)
    return (f"dims={inp['dims']} min|sigma pre|={np.abs(pre).min():.2e} sigma>0: {(pre > 0).mean():.2f} "
            f"|latent grad|={fixture['latent_grad_norm']:.3e} |gen grad|={fixture['gen_grad_norm']:.3e} whole={gen_grad_stored_whole(cfg)}")


def main():
    out_dir = ROOT / "tests" / "golden"
    only = [a.split("=", 1)[1] for a in sys.argv if a.startswith("--case=")]
    for name, cfg in CASES.items():
        if only and name not in only:
            continue
        t0 = time.time()
        msg = gen(name, cfg, out_dir)
        path = out_dir / f"{name}.npz"
        assert path.stat().st_size < 1_000_000, path
        print(f"{name}: {cfg['index_interp']}/{cfg['index_padding']} {msg} -> {path.name} {path.stat().st_size / 1e3:.1f} kB ({time.time() - t0:.1f}s)")


if __name__ == "__main__":
    main()
