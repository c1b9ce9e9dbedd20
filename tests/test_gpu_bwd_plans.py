"""GPU tests of the launch plans of the two key-owner backward kernels (csrc/cpb_regions.h region_bwd_plan; csrc/deform_common.h
dkv_parts / dkv_grid).

region_bwd_plan gives cpb_region_bwd_kernel workgroups of 12 waves = nkbg key blocks x wpk waves per key block, nkbg a divisor of 12 with
no padding of the nkb = ceil(J / 64) key blocks, the remaining key blocks in groups with workgroups of their own.  The key counts below
reach every branch of that rule (N = 196 queries = 7 tiles in one chunk):

    J     nkb   nkbg  groups  wpk
    64     1     1      1     12 -> 7 (clamped by the tile count)
    130    3     3      1      4
    300    5     1      5     12 -> 7
    625   10     2      5      6     (the headline's key count)
    700   11     1     11     12 -> 7
    800   13     1     13     12 -> 7 (above 768 keys)

The 196 queries are one chunk here (region_bwd_plan leaves every wave of a workgroup a tile before it adds chunks); one more case at
400 queries runs two chunks x five key groups.  dkv_parts cuts the
queries of deform_attn_bwd_dkv_kernel into slices whose partial dk / dv go to slabs; its cases (3 bags x 8 heads, 200 queries) run with
7 slices, so that several slabs are summed.

No new tolerance: the region core is held against the per-pair MLP kernels at the bounds of tests/test_gpu_regions.py (helpers shared with
it), the 16-bit mode at those of its 16-bit test, dk / dv against the composed torch reference under tests/test_gpu_parity.py's rule."""
import pytest
import torch

import helpers
from helpers import assert_calibrated, smml
from test_gpu_parity import _core_reference
from test_gpu_regions import NAMES, _problem, _run
from test_gpu_regions_multihead import _first_head_of_each_group, _problem as _problem_mh, _run as _run_mh

pytestmark = pytest.mark.gpu
Fh = smml.functional
S = 14                       # 14 x 14 query grid: 196 queries, 7 tiles of 32 with a ragged last one
KEYS = (64, 130, 300, 625, 700, 800)
_cache = {}


def _grid(side):
    ax = 2.0 * torch.arange(side, dtype=torch.float32) / (side - 1) - 1.0
    return torch.stack((ax.view(1, side).expand(side, side), ax.view(side, 1).expand(side, side)), dim=-1).reshape(side * side, 2).contiguous()


def _case(cuda, J):
    """Inputs of one key count, the per-pair kernels' results and the region kernels' (all regions LDS-resident): computed once, read only."""
    if J not in _cache:
        gen = torch.Generator().manual_seed(700 + J)
        t = _problem(gen, 1, S * S, J, 2)
        t["gq"] = _grid(S)
        wo = torch.randn(1, S * S, 128, generator=gen).to(cuda)
        _cache[J] = (t, wo, _run(t, cuda, wo, False, 0.1, heads=2), _run(t, cuda, wo, True, 0.1, heads=2))
    return _cache[J]


@pytest.mark.parametrize("lds_cap", [0, 96])
@pytest.mark.parametrize("J", KEYS)
def test_region_bias_backward_at_every_branch_of_the_plan(cuda, J, lds_cap):
    """One bag, two heads (one per offset group), 196 queries on a grid: the region kernels against the per-pair MLP kernels at the bounds of
    test_region_core_matches_per_pair_mlp, twice with equal bits; with region_lds_cap lowered (regions beyond the 96th in the global
    accumulators) also against the LDS-resident run at that test's bounds."""
    t, wo, pair, reg = _case(cuda, J)
    Fh.REGION_LDS_CAP = lds_cap
    try:
        a = _run(t, cuda, wo, True, 0.1, heads=2)
        a2 = _run(t, cuda, wo, True, 0.1, heads=2)
    finally:
        Fh.REGION_LDS_CAP = 0
    errs = {}
    for n in a:
        errs[n] = float((a[n] - pair[n]).abs().max()) / max(float(pair[n].abs().max()), 1e-30)
    print(f"J {J} lds_cap {lds_cap}: " + " ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    for n in a:
        assert torch.equal(a[n], a2[n]), f"J {J}: {n} is not run-to-run identical"
    for n in a:
        if n == "b3" or float(pair[n].abs().max()) < 1e-9:
            continue
        tol = 2e-5 if n in ("out", "q", "k", "v") else 5e-4
        if J > 768 and n not in ("out", "q", "k", "v"):
            tol = 2e-2 if n == "vs" else 2e-3
        assert errs[n] <= tol, f"J {J}: {n} differs by {errs[n]:.2e} of its scale between the region and the per-pair kernels"
    if lds_cap:
        for n in a:
            err = float((a[n] - reg[n]).abs().max()) / max(float(reg[n].abs().max()), 1e-30)
            tol = 0.0 if n == "out" else (2e-6 if n in ("q", "k", "v") else 2e-5)
            assert err <= tol, f"J {J}: {n} differs by {err:.2e} between LDS-resident and global-memory regions"


def _assert_against_per_pair(tag, a, b, J):
    """The bounds of test_region_core_matches_per_pair_mlp, every figure printed first."""
    errs = {n: float((a[n] - b[n]).abs().max()) / max(float(b[n].abs().max()), 1e-30) for n in a}
    print(f"{tag}: " + " ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    for n in a:
        if n == "b3" or float(b[n].abs().max()) < 1e-9:
            continue
        tol = 2e-5 if n in ("out", "q", "k", "v") else 5e-4
        if J > 768 and n not in ("out", "q", "k", "v"):
            tol = 2e-2 if n == "vs" else 2e-3
        assert errs[n] <= tol, f"{tag}: {n} differs by {errs[n]:.2e} of its scale between the region and the per-pair kernels"


def test_region_bias_backward_two_heads_per_group(cuda):
    """The headline's key count with two heads per offset group (cpb_region_bwd_kernel<float, true>), twice with equal bits: every output
    against the per-pair kernels at the bounds above, and (an addition) against plain torch in fp64 with the kernels' decisions imposed,
    the rule of test_gpu_regions_multihead.py::test_core_vs_fp64_with_imposed_decisions.
    The per-pair comparison depends on the inputs at so few queries per key: where the two kernel families decide ONE pair differently
    (a pre-activation within rounding of zero) it shows in d vs and the MLP gradients.  Of ten input draws at 196 queries (five key
    counts x two seeds) seven agree to <= 8e-6 in all of them, as this one does (d vs 3.6e-07); the others read d vs 2.2e-04 (130 keys),
    8.1e-04 (625 keys, generator seed 811) and 3.8e-03 (700 keys).  The figures come out the same with the library of the commit before
    the 12-wave plan: they belong to the inputs, not to the launch plan."""
    B, N, J, H, G = 1, S * S, 625, 4, 2
    gen = torch.Generator().manual_seed(811 + J)
    t = _problem_mh(gen, B, N, J, H, G)
    t["gq"] = _grid(S)
    wo = torch.randn(B, N, H * 64, generator=gen)
    a, tapped = _run_mh(t, cuda, wo.to(cuda), H, G, True, 0.1, tap=True)
    a2 = _run_mh(t, cuda, wo.to(cuda), H, G, True, 0.1)
    b = _run_mh(t, cuda, wo.to(cuda), H, G, False, 0.1)
    for n in a:
        assert torch.equal(a[n], a2[n]), f"{n} is not run-to-run identical"
    _assert_against_per_pair("two heads per group", a, b, J)
    m1, m2 = helpers.decisions_of(_first_head_of_each_group(tapped[0]), cuda)
    keep = Fh.deform_attention_dropout_mask(B, N, J, H, 0.1, 3, cuda)
    refs = {}
    for dt in (torch.float32, torch.float64):
        r = {n: x.to(cuda, dt).requires_grad_() for n, x in t.items()}
        o = _core_reference(*(r[n] for n in NAMES), H, G, 0.125, keep, 1.0 / 0.9, masks=(m1, m2))
        (o * wo.to(cuda, dt)).sum().backward()
        refs[dt] = (o, r)
    assert_calibrated("plans two heads per group out", a["out"], refs[torch.float32][0], refs[torch.float64][0])
    for n in t:
        if n != "gq":
            assert_calibrated("plans two heads per group d" + n, a[n], refs[torch.float32][1][n].grad, refs[torch.float64][1][n].grad)


def test_region_bias_backward_several_chunks_and_key_groups(cuda):
    """400 queries (20 x 20: 13 tiles) and 625 keys: two query chunks x five key groups, grid.x = chunks * groups with the d vs slab
    indexed by the chunk - the combination the 196-query cases above (one chunk) do not reach.  Twice with equal bits; against the
    per-pair kernels at the bounds above, and against plain torch in fp64 with the kernels' decisions imposed (the rule of
    test_region_core_vs_fp64_with_imposed_decisions), which does not depend on the draw.
    The per-pair comparison does (see the two-heads case): of four draws at this shape (generator seeds 700 .. 703 + 625) this one agrees to
    <= 5e-6 in every tensor (d vs 3.4e-07); 702 stays inside the bounds (d vs 3.4e-04), 700 and 701 have a pair decided differently
    that shows above them (d b2 8.4e-04, d w2 5.7e-04) - the same figures, digit for digit, with the library of the commit before."""
    side, J = 20, 625
    N = side * side
    gen = torch.Generator().manual_seed(703 + J)
    t = _problem(gen, 1, N, J, 2)
    t["gq"] = _grid(side)
    wo = torch.randn(1, N, 128, generator=gen)
    a, tapped = _run(t, cuda, wo.to(cuda), True, 0.1, heads=2, tap=True)
    a2 = _run(t, cuda, wo.to(cuda), True, 0.1, heads=2)
    b = _run(t, cuda, wo.to(cuda), False, 0.1, heads=2)
    for n in a:
        assert torch.equal(a[n], a2[n]), f"{n} is not run-to-run identical"
    _assert_against_per_pair("two chunks x five key groups", a, b, J)
    m1, m2 = helpers.decisions_of(tapped[0], cuda)
    keep = Fh.deform_attention_dropout_mask(1, N, J, 2, 0.1, 3, cuda)
    refs = {}
    for dt in (torch.float32, torch.float64):
        r = {n: x.to(cuda, dt).requires_grad_() for n, x in t.items()}
        o = _core_reference(*(r[n] for n in NAMES), 2, 2, 0.125, keep, 1.0 / 0.9, masks=(m1, m2))
        (o * wo.to(cuda, dt)).sum().backward()
        refs[dt] = (o, r)
    assert_calibrated("plans two chunks out", a["out"], refs[torch.float32][0], refs[torch.float64][0])
    for n in t:
        if n not in ("gq", "b3"):
            assert_calibrated("plans two chunks d" + n, a[n], refs[torch.float32][1][n].grad, refs[torch.float64][1][n].grad)


def test_region_bias_backward_bf16_mode(cuda):
    """The headline's key count in the bf16 compute mode (cpb_region_bwd_kernel<unsigned short>): against the fp32-grade region kernels at
    the bounds of test_region_core_in_the_16bit_modes, twice with equal bits."""
    t, wo, _, reg = _case(cuda, 625)
    a = _run(t, cuda, wo, True, 0.1, heads=2, compute_dtype="bf16")
    a2 = _run(t, cuda, wo, True, 0.1, heads=2, compute_dtype="bf16")
    for n in a:
        assert torch.equal(a[n], a2[n]), f"{n} is not run-to-run identical"
    for n in a:
        if n == "b3" or float(reg[n].abs().max()) < 1e-9:
            continue
        err = float((a[n] - reg[n]).abs().max()) / max(float(reg[n].abs().max()), 1e-30)
        print(f"bf16: {n} {err:.2e}")
        tol = 1.5e-2 if n == "out" else (3e-2 if n in ("q", "k", "v", "vs") else 6e-2)
        assert err <= tol, f"{n} differs by {err:.2e} of its scale from the fp32-grade region kernels"


@pytest.mark.parametrize("J", [33, 625])
def test_dk_dv_with_several_query_slices(cuda, J):
    """3 bags x 8 heads, 200 queries: dk / dv (and the rest of the fused core) against plain torch in fp64 with the kernels' decisions
    imposed, under the rule of test_fused_core_random_shapes; twice with equal bits."""
    gen = torch.Generator().manual_seed(900 + J)
    B, N, H = 3, 200, 8
    t = _problem(gen, B, N, J, H)
    wo = torch.randn(B, N, H * 64, generator=gen)
    res, tapped = _run(t, cuda, wo.to(cuda), True, 0.25, seed=23, tap=True)
    res2 = _run(t, cuda, wo.to(cuda), True, 0.25, seed=23)
    for n in res:
        assert torch.equal(res[n], res2[n]), f"{n} is not run-to-run identical"
    m1, m2 = helpers.decisions_of(tapped[0], cuda)
    keep = Fh.deform_attention_dropout_mask(B, N, J, H, 0.25, 23, cuda)
    refs = {}
    for dt in (torch.float32, torch.float64):
        r = {n: x.to(cuda, dt).requires_grad_() for n, x in t.items()}
        o = _core_reference(*(r[n] for n in NAMES), H, H, 0.125, keep, 1.0 / 0.75, masks=(m1, m2))
        (o * wo.to(cuda, dt)).sum().backward()
        refs[dt] = (o, r)
    tag = f"dkv {B}x{N}x{J}"
    assert_calibrated(tag + " out", res["out"], refs[torch.float32][0], refs[torch.float64][0])
    for n in ("k", "v", "q", "vs"):
        assert_calibrated(tag + " d" + n, res[n], refs[torch.float32][1][n].grad, refs[torch.float64][1][n].grad)
