"""Host tests (no GPU) of the renderer's inference plan: the route value ``NeRFRendererDGS._resolve`` settles once per call and the one
entry-point resolver ``_entry`` that turns it into a C function and its argument list, on CPU stub models.

Where the expected values come from: every row of ``PARENT`` was taken by evaluating, on the same stubs, the helpers of the commit
before the route value existed -- ``_route`` (its ``effective_precision`` and its warning), ``_use_gen``, ``_use_gen_f16``,
``_gen_call`` (names, the arguments after the scene, the trailing arguments) and ``_gen_route``; for the standard kernels, whose launch
was written inline then, ``_latent_index`` and ``PRECISIONS`` as ``forward()`` / ``render_points()`` / ``_render_image()`` used them.
They are written out here and never computed from the code under test."""
import ctypes as C
import warnings

import pytest
import torch

SHAPES = {"std": {}, "h128_c2": dict(d_hidden=128, n_blocks=4, combine_layer=2), "h128_c0": dict(d_hidden=128, n_blocks=4, combine_layer=0)}
LOOKUPS = {"bilinear/border": ("bilinear", "border"), "nearest/zeros": ("nearest", "zeros"), "bicubic/reflection": ("bicubic", "reflection")}
STEMS = ("render_points", "render", "render_image")

# (shape, lookup, precision, f16x3_any_shape, _force_gen, f16_ok) ->
#   (last_route, effective_precision, the entry points' suffix after diner_<stem>, the arguments between the scene and the shape / packed
#    image -- (interp, padding) stands for a DinerLatentIndex pointer --, the op binding is eligible, precision warnings of the first call,
#    and with lin_z maps: last_route, the argument after the scene, the trailing (precision, bicubic padding) before the maps;
#    on the standard kernels instead: None, None, (the precision argument,))
PARENT = {
    ('std', 'bilinear/border', 'f16x3', False, False, True): ('points_mlp_f16', 'f16x3', '', (), True, 0, None, None, (1,)),
    ('std', 'bilinear/border', 'f16x3', True, False, True): ('points_mlp_f16', 'f16x3', '', (), True, 0, None, None, (1,)),
    ('std', 'bilinear/border', 'f16x3', True, False, False): ('points_mlp_f16', 'f16x3', '', (), True, 0, None, None, (1,)),
    ('std', 'bilinear/border', 'f16x3', True, True, True): ('points_mlp_gen', 'fp32', '_gen', (), False, 1, 'points_mlp_gen_lz', (None,), (0, -1)),
    ('std', 'bilinear/border', 'fp32', False, False, True): ('points_mlp', 'fp32', '', (), True, 0, None, None, (0,)),
    ('std', 'bilinear/border', 'fp32', True, False, True): ('points_mlp', 'fp32', '', (), True, 0, None, None, (0,)),
    ('std', 'bilinear/border', 'fp32', True, True, True): ('points_mlp_gen', 'fp32', '_gen', (), False, 0, 'points_mlp_gen_lz', (None,), (0, -1)),
    ('std', 'nearest/zeros', 'f16x3', False, False, True): ('points_mlp_f16', 'f16x3', '_ix', ((1, 1),), False, 0, None, None, (1,)),
    ('std', 'nearest/zeros', 'f16x3', True, False, True): ('points_mlp_f16', 'f16x3', '_ix', ((1, 1),), False, 0, None, None, (1,)),
    ('std', 'nearest/zeros', 'f16x3', True, False, False): ('points_mlp_f16', 'f16x3', '_ix', ((1, 1),), False, 0, None, None, (1,)),
    ('std', 'nearest/zeros', 'f16x3', True, True, True): ('points_mlp_gen', 'fp32', '_gen_ix', ((1, 1),), False, 1, 'points_mlp_gen_lz', ((1, 1),), (0, -1)),
    ('std', 'nearest/zeros', 'fp32', False, False, True): ('points_mlp', 'fp32', '_ix', ((1, 1),), False, 0, None, None, (0,)),
    ('std', 'nearest/zeros', 'fp32', True, False, True): ('points_mlp', 'fp32', '_ix', ((1, 1),), False, 0, None, None, (0,)),
    ('std', 'nearest/zeros', 'fp32', True, True, True): ('points_mlp_gen', 'fp32', '_gen_ix', ((1, 1),), False, 0, 'points_mlp_gen_lz', ((1, 1),), (0, -1)),
    ('std', 'bicubic/reflection', 'f16x3', False, False, True): ('points_mlp_gen', 'fp32', '_gen_bc', (2,), False, 1, 'points_mlp_gen_lz', (None,), (0, 2)),
    ('std', 'bicubic/reflection', 'f16x3', True, False, True): ('points_mlp_gen_f16', 'f16x3', '_gen_f16_bc', (2,), False, 0, 'points_mlp_gen_f16_lz', (None,), (1, 2)),
    ('std', 'bicubic/reflection', 'f16x3', True, False, False): ('points_mlp_gen', 'fp32', '_gen_bc', (2,), False, 1, 'points_mlp_gen_lz', (None,), (0, 2)),
    ('std', 'bicubic/reflection', 'f16x3', True, True, True): ('points_mlp_gen', 'fp32', '_gen_bc', (2,), False, 1, 'points_mlp_gen_lz', (None,), (0, 2)),
    ('std', 'bicubic/reflection', 'fp32', False, False, True): ('points_mlp_gen', 'fp32', '_gen_bc', (2,), False, 0, 'points_mlp_gen_lz', (None,), (0, 2)),
    ('std', 'bicubic/reflection', 'fp32', True, False, True): ('points_mlp_gen', 'fp32', '_gen_bc', (2,), False, 0, 'points_mlp_gen_lz', (None,), (0, 2)),
    ('std', 'bicubic/reflection', 'fp32', True, True, True): ('points_mlp_gen', 'fp32', '_gen_bc', (2,), False, 0, 'points_mlp_gen_lz', (None,), (0, 2)),
    ('h128_c2', 'bilinear/border', 'f16x3', False, False, True): ('points_mlp_gen', 'fp32', '_gen', (), False, 1, 'points_mlp_gen_lz', (None,), (0, -1)),
    ('h128_c2', 'bilinear/border', 'f16x3', True, False, True): ('points_mlp_gen_f16', 'f16x3', '_gen_f16', (), False, 0, 'points_mlp_gen_f16_lz', (None,), (1, -1)),
    ('h128_c2', 'bilinear/border', 'f16x3', True, False, False): ('points_mlp_gen', 'fp32', '_gen', (), False, 1, 'points_mlp_gen_lz', (None,), (0, -1)),
    ('h128_c2', 'bilinear/border', 'f16x3', True, True, True): ('points_mlp_gen', 'fp32', '_gen', (), False, 1, 'points_mlp_gen_lz', (None,), (0, -1)),
    ('h128_c2', 'bilinear/border', 'fp32', False, False, True): ('points_mlp_gen', 'fp32', '_gen', (), False, 0, 'points_mlp_gen_lz', (None,), (0, -1)),
    ('h128_c2', 'bilinear/border', 'fp32', True, False, True): ('points_mlp_gen', 'fp32', '_gen', (), False, 0, 'points_mlp_gen_lz', (None,), (0, -1)),
    ('h128_c2', 'bilinear/border', 'fp32', True, True, True): ('points_mlp_gen', 'fp32', '_gen', (), False, 0, 'points_mlp_gen_lz', (None,), (0, -1)),
    ('h128_c2', 'nearest/zeros', 'f16x3', False, False, True): ('points_mlp_gen', 'fp32', '_gen_ix', ((1, 1),), False, 1, 'points_mlp_gen_lz', ((1, 1),), (0, -1)),
    ('h128_c2', 'nearest/zeros', 'f16x3', True, False, True): ('points_mlp_gen_f16', 'f16x3', '_gen_f16_ix', ((1, 1),), False, 0, 'points_mlp_gen_f16_lz', ((1, 1),), (1, -1)),
    ('h128_c2', 'nearest/zeros', 'f16x3', True, False, False): ('points_mlp_gen', 'fp32', '_gen_ix', ((1, 1),), False, 1, 'points_mlp_gen_lz', ((1, 1),), (0, -1)),
    ('h128_c2', 'nearest/zeros', 'f16x3', True, True, True): ('points_mlp_gen', 'fp32', '_gen_ix', ((1, 1),), False, 1, 'points_mlp_gen_lz', ((1, 1),), (0, -1)),
    ('h128_c2', 'nearest/zeros', 'fp32', False, False, True): ('points_mlp_gen', 'fp32', '_gen_ix', ((1, 1),), False, 0, 'points_mlp_gen_lz', ((1, 1),), (0, -1)),
    ('h128_c2', 'nearest/zeros', 'fp32', True, False, True): ('points_mlp_gen', 'fp32', '_gen_ix', ((1, 1),), False, 0, 'points_mlp_gen_lz', ((1, 1),), (0, -1)),
    ('h128_c2', 'nearest/zeros', 'fp32', True, True, True): ('points_mlp_gen', 'fp32', '_gen_ix', ((1, 1),), False, 0, 'points_mlp_gen_lz', ((1, 1),), (0, -1)),
    ('h128_c2', 'bicubic/reflection', 'f16x3', False, False, True): ('points_mlp_gen', 'fp32', '_gen_bc', (2,), False, 1, 'points_mlp_gen_lz', (None,), (0, 2)),
    ('h128_c2', 'bicubic/reflection', 'f16x3', True, False, True): ('points_mlp_gen_f16', 'f16x3', '_gen_f16_bc', (2,), False, 0, 'points_mlp_gen_f16_lz', (None,), (1, 2)),
    ('h128_c2', 'bicubic/reflection', 'f16x3', True, False, False): ('points_mlp_gen', 'fp32', '_gen_bc', (2,), False, 1, 'points_mlp_gen_lz', (None,), (0, 2)),
    ('h128_c2', 'bicubic/reflection', 'f16x3', True, True, True): ('points_mlp_gen', 'fp32', '_gen_bc', (2,), False, 1, 'points_mlp_gen_lz', (None,), (0, 2)),
    ('h128_c2', 'bicubic/reflection', 'fp32', False, False, True): ('points_mlp_gen', 'fp32', '_gen_bc', (2,), False, 0, 'points_mlp_gen_lz', (None,), (0, 2)),
    ('h128_c2', 'bicubic/reflection', 'fp32', True, False, True): ('points_mlp_gen', 'fp32', '_gen_bc', (2,), False, 0, 'points_mlp_gen_lz', (None,), (0, 2)),
    ('h128_c2', 'bicubic/reflection', 'fp32', True, True, True): ('points_mlp_gen', 'fp32', '_gen_bc', (2,), False, 0, 'points_mlp_gen_lz', (None,), (0, 2)),
    ('h128_c0', 'bilinear/border', 'f16x3', False, False, True): ('points_mlp_gen', 'fp32', '_gen', (), False, 1, 'points_mlp_gen_lz', (None,), (0, -1)),
    ('h128_c0', 'bilinear/border', 'f16x3', True, False, True): ('points_mlp_gen_f16', 'f16x3', '_gen_f16', (), False, 0, 'points_mlp_gen_f16_lz', (None,), (1, -1)),
    ('h128_c0', 'bilinear/border', 'f16x3', True, False, False): ('points_mlp_gen', 'fp32', '_gen', (), False, 1, 'points_mlp_gen_lz', (None,), (0, -1)),
    ('h128_c0', 'bilinear/border', 'f16x3', True, True, True): ('points_mlp_gen', 'fp32', '_gen', (), False, 1, 'points_mlp_gen_lz', (None,), (0, -1)),
    ('h128_c0', 'bilinear/border', 'fp32', False, False, True): ('points_mlp_gen', 'fp32', '_gen', (), False, 0, 'points_mlp_gen_lz', (None,), (0, -1)),
    ('h128_c0', 'bilinear/border', 'fp32', True, False, True): ('points_mlp_gen', 'fp32', '_gen', (), False, 0, 'points_mlp_gen_lz', (None,), (0, -1)),
    ('h128_c0', 'bilinear/border', 'fp32', True, True, True): ('points_mlp_gen', 'fp32', '_gen', (), False, 0, 'points_mlp_gen_lz', (None,), (0, -1)),
    ('h128_c0', 'nearest/zeros', 'f16x3', False, False, True): ('points_mlp_gen', 'fp32', '_gen_ix', ((1, 1),), False, 1, 'points_mlp_gen_lz', ((1, 1),), (0, -1)),
    ('h128_c0', 'nearest/zeros', 'f16x3', True, False, True): ('points_mlp_gen_f16', 'f16x3', '_gen_f16_ix', ((1, 1),), False, 0, 'points_mlp_gen_f16_lz', ((1, 1),), (1, -1)),
    ('h128_c0', 'nearest/zeros', 'f16x3', True, False, False): ('points_mlp_gen', 'fp32', '_gen_ix', ((1, 1),), False, 1, 'points_mlp_gen_lz', ((1, 1),), (0, -1)),
    ('h128_c0', 'nearest/zeros', 'f16x3', True, True, True): ('points_mlp_gen', 'fp32', '_gen_ix', ((1, 1),), False, 1, 'points_mlp_gen_lz', ((1, 1),), (0, -1)),
    ('h128_c0', 'nearest/zeros', 'fp32', False, False, True): ('points_mlp_gen', 'fp32', '_gen_ix', ((1, 1),), False, 0, 'points_mlp_gen_lz', ((1, 1),), (0, -1)),
    ('h128_c0', 'nearest/zeros', 'fp32', True, False, True): ('points_mlp_gen', 'fp32', '_gen_ix', ((1, 1),), False, 0, 'points_mlp_gen_lz', ((1, 1),), (0, -1)),
    ('h128_c0', 'nearest/zeros', 'fp32', True, True, True): ('points_mlp_gen', 'fp32', '_gen_ix', ((1, 1),), False, 0, 'points_mlp_gen_lz', ((1, 1),), (0, -1)),
    ('h128_c0', 'bicubic/reflection', 'f16x3', False, False, True): ('points_mlp_gen', 'fp32', '_gen_bc', (2,), False, 1, 'points_mlp_gen_lz', (None,), (0, 2)),
    ('h128_c0', 'bicubic/reflection', 'f16x3', True, False, True): ('points_mlp_gen_f16', 'f16x3', '_gen_f16_bc', (2,), False, 0, 'points_mlp_gen_f16_lz', (None,), (1, 2)),
    ('h128_c0', 'bicubic/reflection', 'f16x3', True, False, False): ('points_mlp_gen', 'fp32', '_gen_bc', (2,), False, 1, 'points_mlp_gen_lz', (None,), (0, 2)),
    ('h128_c0', 'bicubic/reflection', 'f16x3', True, True, True): ('points_mlp_gen', 'fp32', '_gen_bc', (2,), False, 1, 'points_mlp_gen_lz', (None,), (0, 2)),
    ('h128_c0', 'bicubic/reflection', 'fp32', False, False, True): ('points_mlp_gen', 'fp32', '_gen_bc', (2,), False, 0, 'points_mlp_gen_lz', (None,), (0, 2)),
    ('h128_c0', 'bicubic/reflection', 'fp32', True, False, True): ('points_mlp_gen', 'fp32', '_gen_bc', (2,), False, 0, 'points_mlp_gen_lz', (None,), (0, 2)),
    ('h128_c0', 'bicubic/reflection', 'fp32', True, True, True): ('points_mlp_gen', 'fp32', '_gen_bc', (2,), False, 0, 'points_mlp_gen_lz', (None,), (0, 2)),
}

_MODELS = {}


def _model(shape, lookup):
    """the CPU stub of (shape, lookup) on an 8 x 8, 2-view scene, built once and never modified"""
    if (shape, lookup) not in _MODELS:
        from synthetic import synth
        from synthetic.model_stub import model_from_scene
        d = dict(d_latent=512, d_hidden=512, n_blocks=5, combine_layer=3)
        d.update(SHAPES[shape])
        interp, padding = LOOKUPS[lookup]
        _MODELS[shape, lookup] = model_from_scene(synth.make_scene(8, 8, 2, seed=0, feature_padding=2), synth.make_mlp_weights(1, d_in=55, **d),
                                                  device="cpu", index_interp=interp, index_padding=padding, **d)
    return _MODELS[shape, lookup]


def _renderer(lookup, precision, any_shape, force):
    from diner_amd import NeRFRendererDGS
    r = NeRFRendererDGS(f16x3_any_shape=any_shape, bicubic_index=lookup.startswith("bicubic"))
    r.precision, r._force_gen = precision, force
    return r


_BYREF = type(C.byref(C.c_int()))


def _plain(args, sc, packed):
    """an argument list with ctypes' wrappers taken off: "sc" / "packed" for the two fixed ones, (interp, padding) for a DinerLatentIndex
    pointer, ("shape", the struct's fields) for a DinerMlpShape pointer, the address of a pointer"""
    from diner_amd import _lib
    out = []
    for a in args:
        if isinstance(a, _BYREF):
            o = a._obj
            if o is sc:
                out.append("sc")
            elif isinstance(o, _lib.DinerLatentIndex):
                out.append((o.interp, o.padding))
            else:
                assert isinstance(o, _lib.DinerMlpShape)
                out.append(("shape", o.d_in, o.d_latent, o.d_hidden, o.n_blocks, o.combine_layer, o.num_freqs))
        elif isinstance(a, C.c_void_p):
            out.append("packed" if a.value == packed.data_ptr() else a.value)
        else:
            out.append(a)
    return out


@pytest.mark.parametrize("key", list(PARENT), ids=lambda k: "-".join(str(v) for v in k))
def test_route_and_entry_points_are_the_parents(key):
    from diner_amd import _lib
    shape, lookup, precision, any_shape, force, f16_ok = key
    route_name, eff, suffix, look, op_ok, n_warn, lz_route, lz_look, tail = PARENT[key]
    m = _model(shape, lookup)
    r = _renderer(lookup, precision, any_shape, force)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        route = r._resolve(m, f16_ok=f16_ok)
        r._resolve(m, f16_ok=f16_ok)                                   # the warning comes once per renderer
    assert len(w) == n_warn and all(issubclass(x.category, UserWarning) and "runs in exact fp32" in str(x.message) for x in w)
    d = dict(d_hidden=512, n_blocks=5, combine_layer=3)
    d.update(SHAPES[shape])
    assert tuple(route.shape) == (55, 512, d["d_hidden"], d["n_blocks"], d["combine_layer"], 6, 0.0)
    assert (route.stem, route.effective_precision, route.op_ok) == (route_name, eff, op_ok)
    assert route.gen == ("_gen" in suffix) and route.f16 == ("_f16" in suffix)
    # _route: the same settlement for the callers that want the shape, effective_precision set
    r2 = _renderer(lookup, precision, any_shape, force)
    with warnings.catch_warnings(record=True) as w2:
        warnings.simplefilter("always")
        assert r2._route(m, f16_ok=f16_ok) == route.shape
    assert r2.effective_precision == eff and len(w2) == n_warn
    # the entry points of the three stems, and where the route-dependent arguments stand
    sc, packed, scratch, lz = _lib.DinerScene(), torch.zeros(4), torch.zeros(4), torch.zeros(4)
    shape_arg = ("shape", 55, 512, d["d_hidden"], d["n_blocks"], d["combine_layer"], 6)
    for stem in STEMS:
        fn, name, args = r._entry(route, stem, None, sc, packed, ("a0", "a1"), ("b0", "b1"), scratch)
        assert name == "diner_" + stem + suffix and fn is getattr(_lib.lib(), name)
        got = _plain(args, sc, packed)
        if route.gen:
            assert got == ["sc", *look, shape_arg, "packed", "a0", "a1", "b0", "b1"]
        else:
            mid = [tail[0], scratch.data_ptr()] if stem == "render_points" else [tail[0]]
            assert got == ["sc", *look, "packed", "a0", "a1", *mid, "b0", "b1"]
        if route.gen:
            fn, name, args = r._entry(route, stem, lz, sc, packed, ("a0", "a1"), ("b0", "b1"), scratch)
            assert name == "diner_" + stem + "_gen_lz" and fn is getattr(_lib.lib(), name)
            assert _plain(args, sc, packed) == ["sc", *lz_look, shape_arg, "packed", "a0", "a1", "b0", "b1", *tail, lz.data_ptr()]
    # what the call leaves behind
    r._ran(route, None, "ctypes")
    assert (r.last_route, r.last_binding, r.effective_precision) == (route_name, "ctypes", eff)
    if route.gen:
        r._ran(route, lz, "ctypes")
        assert (r.last_route, r.last_binding, r.effective_precision) == (lz_route, "ctypes", eff)
    elif op_ok:
        r._ran(route, None, "torch_ops")
        assert (r.last_route, r.last_binding) == (route_name, "torch_ops")


def test_maps_are_wanted_outside_grad_mode_for_a_shape_with_lin_z_only():
    """the one statement of "this call reads shape-general lin_z maps": the switch, no grad mode (even when nothing requires grad), and
    a lin_z layer -- combine_layer = 0 has none and never uses maps"""
    from diner_amd import NeRFRendererDGS
    on, off = NeRFRendererDGS(linz_maps_any_shape=True), NeRFRendererDGS()
    c2, c0 = (NeRFRendererDGS._validate_model(_model(s, "bilinear/border")) for s in ("h128_c2", "h128_c0"))
    with torch.no_grad():
        assert on._linz_gen_wanted(c2) is True and on._linz_gen_wanted(c0) is False and off._linz_gen_wanted(c2) is False
    with torch.enable_grad():
        assert on._linz_gen_wanted(c2) is False


def test_the_scene_tensors_keep_their_six_places_and_name_the_maps():
    from diner_amd.renderer import _Keep
    assert _Keep._fields == ("maps", "poses", "focal", "c", "latent", "linz", "linz_gen")
    k = _Keep(0, 1, 2, 3, 4, 5)
    assert k[4] == 4 and k.linz_gen is None and tuple(k[:6]) == (0, 1, 2, 3, 4, 5)


def test_predicates_are_asked_through_the_instance_and_the_model_is_validated_once():
    from diner_amd import NeRFRendererDGS
    m = _model("std", "bilinear/border")
    r = NeRFRendererDGS()
    r.precision = "fp32"
    assert not r._resolve(m).gen
    r._needs_gen = lambda shape, model=None: True                       # an instance-level override, as tools/bench_bicubic.py sets it
    route = r._resolve(m)
    assert route.gen and route.stem == "points_mlp_gen" and not route.op_ok
    calls = []
    validate = r._validate
    r._validate = lambda model: (calls.append(model), validate(model))[1]
    r._resolve(m)
    assert len(calls) == 1


def test_the_precision_warning_points_at_the_line_that_called_forward():
    """forward() on CPU rays: the route is settled (and the warning given) before the rays are refused"""
    from diner_amd import NeRFRendererDGS
    r = NeRFRendererDGS(n_samples=4, n_depth_candidates=8, n_gaussian=1)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with pytest.raises(RuntimeError, match="GPU only"):
            r.forward(_model("h128_c2", "bilinear/border"), torch.zeros(1, 2, 8))
    assert len(w) == 1 and w[0].category is UserWarning and w[0].filename == __file__
