"""CPU: which core a deform_attention call takes (functional.deform_path), over the cross product of the options that decide it, against
the rules as deform_attention and its autograd Functions applied them before they were gathered into one function."""
import itertools

import pytest

from helpers import smml

Fh = smml.functional

RAW_2D = "the raw-offset position transform (cpb_log_distance=False) exists for 1-D positions without the table modes"
TABLE_RAW = "the table modes are built for the signed-log position transform only"
FWD_NEEDS_16 = "cpb_table belongs to the 16-bit compute modes: pass compute_dtype='bf16' or 'fp16'"
TABLE_NEEDS_16 = "the table mode belongs to the 16-bit compute modes: pass compute_dtype='bf16' or 'fp16'"


def expected(posdim, heads, groups, keys, w3_shape, log_distance, compute_dtype, cpb_table, cpb_regions, pmax_given, capturing, regions_on):
    """The path, or (exception type, message)."""
    if cpb_regions is not None and bool(cpb_regions) and posdim == 1:
        why = None
        if not log_distance:
            why = "raw distances (cpb_log_distance=False)"
        elif compute_dtype is not None:
            why = "the 16-bit compute modes"
        elif cpb_table:
            why = "the table modes"
        elif heads % groups or heads // groups not in (1, 2):
            why = f"heads // groups = {heads // groups} (supported: 1, 2)"
        elif keys > 16384:
            why = f"{keys} keys (at most 16384)"
        elif tuple(w3_shape) != (heads // groups, 32):
            why = "a bias MLP other than 1 -> 32 -> 32 -> heads // groups"
        if why:
            return ValueError, f"cpb_regions=True with 1-D positions: the piece path does not support {why}"
        return "region1d"
    if cpb_table and not log_distance:
        return NotImplementedError, TABLE_RAW
    if cpb_table == "forward":
        return (ValueError, FWD_NEEDS_16) if compute_dtype is None else "pair_table_forward"
    if cpb_table:
        return (ValueError, TABLE_NEEDS_16) if compute_dtype is None else "table"
    use = regions_on if cpb_regions is None else bool(cpb_regions)
    if (use and log_distance and posdim == 2 and heads == groups and keys <= 16384 and tuple(w3_shape) == (1, 32)
            and (pmax_given or not capturing)):
        return "region"
    if not log_distance and posdim != 1:
        return NotImplementedError, RAW_2D
    return "pair"


CASES = list(itertools.product((1, 2), ((8, 8), (8, 4)), (16384, 16385), ((1, 32), (2, 32)), (True, False), (None, "bf16"),
                               (False, "forward", True), (None, False, True), (False, True), (False, True)))


@pytest.mark.parametrize("regions_on", [True, False])
def test_deform_path_matches_the_rules(monkeypatch, regions_on):
    monkeypatch.setattr(Fh, "CPB_REGIONS", regions_on)          # read at call time
    seen = set()
    for posdim, (heads, groups), keys, w3, logd, dt, table, regions, pmax_given, capturing in CASES:
        want = expected(posdim, heads, groups, keys, w3, logd, dt, table, regions, pmax_given, capturing, regions_on)
        kw = dict(posdim=posdim, heads=heads, groups=groups, keys=keys, w2_shape=(32, 32), w3_shape=w3, log_distance=logd, compute_dtype=dt,
                  cpb_table=table, cpb_regions=regions, region_pmax_given=pmax_given, capturing=capturing)
        case = (posdim, heads, groups, keys, w3, logd, dt, table, regions, pmax_given, capturing)
        if isinstance(want, str):
            assert Fh.deform_path(**kw) == want, case
        else:
            with pytest.raises(want[0]) as e:
                Fh.deform_path(**kw)
            assert str(e.value) == want[1], case
        seen.add(want if isinstance(want, str) else want[0])
    assert {"region1d", "region", "pair", "pair_table_forward", "table", ValueError, NotImplementedError} <= seen


def test_deform_path_rejects_unknown_options():
    with pytest.raises(ValueError, match="cpb_table must be False"):
        Fh.deform_path(posdim=2, heads=8, groups=8, keys=64, cpb_table="half")
    with pytest.raises(ValueError, match="compute_dtype must be None"):
        Fh.deform_path(posdim=2, heads=8, groups=8, keys=64, compute_dtype="fp8")
