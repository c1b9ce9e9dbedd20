"""CPU: the deformable-attention launches are bound by parameter name from include/smml.h.  The binder (_capi.bind / _capi.call) on
hand-written prototypes, and the namespaces of functional.py's deform section - their key sets are module constants - against the real
header: every parameter of every entry point a namespace serves is a key of it, and no key is dead."""
import ctypes

import pytest
import torch

from helpers import smml

Fh, capi = smml.functional, smml._capi

PROTOS = """/* two entry points of one family: the second has no `w`, takes `G` and ends in `dtype` */
int smml_t_fwd_f32(const float* q, const float* w, float* out, unsigned short* ids, void* workspace, size_t workspace_bytes, int B, int H,
                   float scale, unsigned long long dropout_seed, void* stream, const SmmlDeformOpts* opts);
int smml_t16_fwd(const float* q, float* out, unsigned short* ids, int B, int H, int G, float scale, int dtype, void* stream,
                 const SmmlDeformOpts* opts);
size_t smml_t_bytes(int B, int H);"""


def parsed():
    params = {}
    sigs = capi.parse_prototypes(PROTOS, params)
    return sigs, params


def test_params_keep_what_the_prototype_says():
    sigs, params = parsed()
    C = ctypes
    assert params["smml_t16_fwd"] == [("q", C.c_void_p, True), ("out", C.c_void_p, True), ("ids", C.c_void_p, False), ("B", C.c_int, False),
                                      ("H", C.c_int, False), ("G", C.c_int, False), ("scale", C.c_float, False), ("dtype", C.c_int, False),
                                      ("stream", C.c_void_p, False), ("opts", C.POINTER(capi.DeformOpts), False)]
    assert params["smml_t_bytes"] == [("B", C.c_int, False), ("H", C.c_int, False)]
    for name, (_, argtypes) in sigs.items():                   # SIGNATURES' shape is unchanged: the types, in order
        assert [t for _, t, _ in params[name]] == argtypes
    assert set(capi.PARAMS) == set(capi.SIGNATURES)
    for name, (_, argtypes) in capi.SIGNATURES.items():
        assert [t for _, t, _ in capi.PARAMS[name]] == argtypes, name
    fwd = capi.PARAMS["smml_deform_attn16_region_fwd"]
    assert [n for n, _, _ in fwd[11:16]] == ["tables", "out", "lse", "logits16", "region_ids"]
    assert [f for _, _, f in fwd[11:16]] == [False, True, True, False, False]      # const void*, float*, float*, unsigned short* x 2


def test_bind_orders_by_the_header_and_ignores_surplus():
    _, params = parsed()
    stream, opts = ctypes.c_void_p(0x1000), ctypes.byref(capi.DeformOpts())
    ns = dict(opts=opts, stream=stream, dtype=1, G=4, scale=0.125, dropout_seed=7, H=8, B=2, workspace_bytes=64, workspace=None, ids=None, out=None,
              w=None, q=None, unused="surplus")
    assert capi.bind("smml_t_fwd_f32", ns, params) == [None, None, None, None, None, 64, 2, 8, 0.125, 7, stream, opts]
    assert capi.bind("smml_t16_fwd", ns, params) == [None, None, None, 2, 8, 4, 0.125, 1, stream, opts]
    assert capi.bind("smml_t16_fwd", dict(reversed(list(ns.items()))), params) == [None, None, None, 2, 8, 4, 0.125, 1, stream, opts]
    assert capi.bind("smml_t_bytes", ns, params) == [2, 8]


def test_bind_names_a_missing_parameter():
    _, params = parsed()
    ns = dict(q=None, out=None, ids=None, B=2, H=8, scale=0.125, dtype=0, stream=None, opts=None)          # no G
    with pytest.raises(RuntimeError, match=r"smml_t16_fwd: no value for its parameter `G`"):
        capi.bind("smml_t16_fwd", ns, params)
    with pytest.raises(RuntimeError, match=r"smml_deform_attn_nst: no value for its parameter `N`"):
        capi.bind("smml_deform_attn_nst", {"n": 1})                                                         # the real header's plan


def test_bind_converts_tensors_by_the_parameter_type():
    _, params = parsed()
    ns = dict(q=torch.zeros(4, dtype=torch.float64), out=None, ids=None, B=2, H=8, G=4, scale=0.125, dtype=0, stream=None, opts=None)
    with pytest.raises(RuntimeError, match="smml fp32 kernel got dtype torch.float64"):                     # fptr's check, from `const float*`
        capi.bind("smml_t16_fwd", ns, params)
    with pytest.raises(RuntimeError) as fp32_on_cpu:
        capi.fptr(torch.zeros(4))
    with pytest.raises(RuntimeError) as bound:                                                              # fp32 passes fptr's check, then ptr's
        capi.bind("smml_t16_fwd", dict(ns, q=torch.zeros(4)), params)
    assert str(bound.value) == str(fp32_on_cpu.value) and "GPU HBM" in str(bound.value)
    with pytest.raises(RuntimeError) as int16_on_cpu:                                                       # `unsigned short*`: ptr, no fp32 check
        capi.bind("smml_t16_fwd", dict(ns, q=None, ids=torch.zeros(4, dtype=torch.int16)), params)
    assert str(int16_on_cpu.value) == str(fp32_on_cpu.value)
    assert capi.bind("smml_t16_fwd", dict(ns, q=None), params)[:3] == [None, None, None]                    # None is NULL


def test_call_holds_the_namespace_to_its_key_set():
    with pytest.raises(RuntimeError, match="smml_deform_attn_nst: the namespace holds"):
        capi.call("smml_deform_attn_nst", {"N": 100, "typo": 1}, frozenset({"N"}))
    assert capi.call("smml_deform_attn_nst", {"N": 2500}, frozenset({"N"})) == 2560
    assert capi.call("smml_deform_attn_nst", {"N": 2500, "surplus": 1}) == 2560


def _names(proto: str):
    return {n for n, _, _ in capi.PARAMS[proto]}


def test_core_namespaces_cover_the_header_and_have_no_dead_key():
    used = {}
    for (path, multi_head, m16) in Fh._CORE_ENTRY:
        fn = "TABLE" if path == "table" else "MLP"
        for kind, proto in zip(("FWD", "BWD", "WS"), Fh.core_entry_points(path, multi_head, m16)):
            keys = getattr(Fh, f"{fn}_{kind}_KEYS")
            assert _names(proto) <= keys, f"{proto}: {sorted(_names(proto) - keys)} missing from {fn}_{kind}_KEYS"
            used.setdefault((fn, kind), set()).update(_names(proto))
    assert len(used) == 6
    for (fn, kind), names in used.items():
        keys = getattr(Fh, f"{fn}_{kind}_KEYS")
        assert keys == names, f"{fn}_{kind}_KEYS: no prototype of its cores takes {sorted(keys - names)}"


def test_core_entry_points_are_the_headers():
    assert len(Fh._CORE_ENTRY) == 10
    assert Fh.core_entry_points("pair", False, False) == ("smml_deform_attn_fwd_f32", "smml_deform_attn_bwd_f32",
                                                          "smml_deform_attn_bwd_workspace_bytes")
    assert Fh.core_entry_points("pair_table_forward", False, True) == ("smml_deform_attn_table_fwd", "smml_deform_attn16_bwd",
                                                                       "smml_deform_attn_bwd_workspace_bytes")
    assert Fh.core_entry_points("region", True, True) == ("smml_deform_attn16_region_mh_fwd", "smml_deform_attn16_region_mh_bwd",
                                                          "smml_deform_attn_region_mh_bwd_workspace_bytes")
    for core in Fh._CORE_ENTRY:
        assert all(n in capi.SIGNATURES for n in Fh.core_entry_points(*core)), core


SINGLE = {"BUILD_KEYS": ("smml_cpb_regions_build", "smml_cpb_regions_mh_build", "smml_cpb_regions1d_build"),
          "WIDE_DECISIONS_KEYS": ("smml_deform_attn_wide_decisions",), "RELU1_KEYS": ("smml_deform_attn_relu1_masks",),
          "DROPOUT_MASK_KEYS": ("smml_deform_attn_dropout_mask_f32",), "MASK_TABLE_KEYS": ("smml_cpb_mask_table",)}


@pytest.mark.parametrize("const", sorted(SINGLE))
def test_single_launch_namespaces_cover_the_header_and_have_no_dead_key(const):
    keys = getattr(Fh, const)
    for proto in SINGLE[const]:
        assert _names(proto) <= keys, f"{proto}: {sorted(_names(proto) - keys)} missing from {const}"
    assert keys == set().union(*(_names(p) for p in SINGLE[const]))
