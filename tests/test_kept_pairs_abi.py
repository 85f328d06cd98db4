"""CPU tests that the two forms of a kept reader family -- the whole-list form and the per-window form: lh_kept_across* /
lh_kept_series*, lh_kept_count_le* / lh_kept_heat*, lh_kept_spread* / lh_kept_spread_series*, lh_kept_compare* / lh_kept_drift* --
share their argument checks: every bad argument the two have in common is given to both, the window form with valid windows, in
each of the four entry forms (rows, ids, and the _device variant of each), and both return the same code and write nothing.  The
handle pointers are fakes that are never dereferenced: all of this is decided on the host before a handle is looked at."""
import numpy as np
import pytest

from tests.test_kept_readers_abi import BIG, _handles, _lists

H2 = _handles(0x1000, 0x2000)                                                 # the good list: two handles
SERIES_WIN = np.array([0, 1, 1, 2, 0, 2], dtype=np.uint32)                    # [lo, hi) of that list
DRIFT_WIN = np.array([0, 1, 1, 2, 0, 2, 0, 2], dtype=np.uint32)               # {base_lo, base_hi, cur_lo, cur_hi}
IDS = np.arange(4, dtype=np.uint32)
P, P33 = np.array([0.5, 0.99, 1.5, np.nan]), np.zeros(33)
BOUNDS, B65 = np.array([-np.inf, -1.0, -0.0, 0.0, 0.25, 0.25, 1e200, np.inf]), np.arange(65.0)
DOWN, NAN = np.array([0.0, 2.0, 1.0]), np.array([0.0, np.nan, 1.0])
# lead: what stands between the rows and the flags; bad_lead: each of the family's own causes of LH_EINVAL there
PCT = dict(lead=(P.ctypes.data, 4),
           bad_lead={"np > LH_MAX_PERCENTILES": (P33.ctypes.data, 33), "NULL p with np > 0": (None, 4),
                     **{f"p off its alignment by {off}": (P.ctypes.data + off, 1) for off in range(1, 8)}})
LE = dict(lead=(BOUNDS.ctypes.data, 8),
          bad_lead={"nb == 0": (BOUNDS.ctypes.data, 0), "nb > LH_MAX_BOUNDS": (B65.ctypes.data, 65), "NULL bounds": (None, 8),
                    "unordered bounds": (DOWN.ctypes.data, 3), "a NaN bound": (NAN.ctypes.data, 3),
                    **{f"bounds off their alignment by {off}": (BOUNDS.ctypes.data + off, 2) for off in range(1, 8)}})
FAMILIES = {
    "across": dict(parent="lh_kept_across", window="lh_kept_series", win=SERIES_WIN, nwin=3, **PCT,
                   outs=dict(count=np.uint64, sum=np.float64, nbuckets=np.uint32, present_bits=np.uint64, pkeys=np.int16,
                             pvalid=np.uint8)),
    "count_le": dict(parent="lh_kept_count_le", window="lh_kept_heat", win=SERIES_WIN, nwin=3, **LE,
                     outs=dict(cum=np.uint64, total=np.uint64)),
    "spread": dict(parent="lh_kept_spread", window="lh_kept_spread_series", win=SERIES_WIN, nwin=3, **PCT,
                   outs=dict(count=np.uint64, sum=np.float64, m2=np.float64, pkeys=np.int16, pvalid=np.uint8, count_le=np.uint64,
                             sum_le=np.float64)),
    "compare": dict(parent="lh_kept_compare", window="lh_kept_drift", win=DRIFT_WIN, nwin=2, lead=(), bad_lead={},
                    outs=dict(count_a=np.uint64, count_b=np.uint64, ks=np.float64, ks_key=np.int16, ks_below_a=np.uint64,
                              ks_below_b=np.uint64, w1=np.float64, shift=np.float64)),
}


def _both(L, fam, ids_form, dev, kept, nkept, ids, n, lead, flags, outs):
    """the codes of the family's two forms for the same arguments: the parent's (lh_kept_compare*: the list as `base` with a good
    `cur`, then as `cur` with a good `base`), and the window form's with valid windows"""
    suffix = ("_ids" if ids_form else "") + ("_device" if dev else "")
    rows = (ids if ids_form else 0, n)
    tail = (*lead, flags, None, *outs)
    parent, window = getattr(L, fam["parent"] + suffix), getattr(L, fam["window"] + suffix)
    if fam["parent"] == "lh_kept_compare":
        if kept is H2 and nkept == 2:                                         # the good list: one handle a side
            got = [parent(_handles(0x1000), 1, _handles(0x2000), 1, *rows, *tail)]
        else:
            one = _handles(0x3000)
            got = [parent(kept, nkept, one, 1, *rows, *tail), parent(one, 1, kept, nkept, *rows, *tail)]
    else:
        got = [parent(kept, nkept, *rows, *tail)]
    return got, window(kept, nkept, fam["win"].ctypes.data, fam["nwin"], *rows, *tail)


def _cases(fam, ids_form, outs, widths):
    """(what is wrong, the arguments) for every bad argument the two forms have in common: each a cause of LH_EINVAL"""
    good = dict(kept=H2, nkept=2, ids=IDS.ctypes.data, lead=fam["lead"], flags=0, outs=outs)
    _, h65, holes = _lists()
    if ids_form:
        yield "NULL ids", dict(good, ids=None)
        for off in (1, 2, 3):
            yield f"ids off their alignment by {off}", dict(good, ids=IDS.ctypes.data + off)
    yield "a NULL list", dict(good, kept=None)
    yield "an empty list", dict(good, nkept=0)
    yield "a list of LH_MAX_KEPT + 1 handles", dict(good, kept=h65, nkept=65)
    for h in holes:
        yield f"a NULL handle in a list of {len(h)}", dict(good, kept=h, nkept=len(h))
    for flags in (1, 2, 0x80000000):
        yield f"flags {flags:#x}", dict(good, flags=flags)
    yield "no output pointer at all", dict(good, outs=[None] * len(outs))
    for j, width in enumerate(widths):
        for off in range(1, width):
            bad = list(outs)
            bad[j] += off
            yield f"output {j} off its alignment by {off}", dict(good, outs=bad)
            yield f"output {j} alone, off its alignment by {off}", dict(good, outs=[b if i == j else None for i, b in enumerate(bad)])
    for what, lead in fam["bad_lead"].items():
        yield what, dict(good, lead=lead)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_two_forms_of_a_family_share_their_checks(native_lib, family):
    from loghisto_amd import _native
    L, EINVAL, ERANGE, fam = native_lib, _native.EINVAL, _native.ERANGE, FAMILIES[family]
    arrays = {k: np.full(32, 7, dtype=t) for k, t in fam["outs"].items()}
    outs, widths = [a.ctypes.data for a in arrays.values()], [a.itemsize for a in arrays.values()]
    good = dict(kept=H2, nkept=2, ids=IDS.ctypes.data, lead=fam["lead"], flags=0, outs=outs)
    seen = set()
    for ids_form in (False, True):
        for dev in (False, True):
            form = (ids_form, dev)
            for what, args in _cases(fam, ids_form, outs, widths):
                seen.add(what.split(" by ")[0])
                # alone, and together with more rows than any engine can have: every LH_EINVAL cause comes before the early LH_ERANGE
                for n in (1, 3, BIG, (1 << 64) - 1):
                    parent, window = _both(L, fam, ids_form, dev, n=n, **args)
                    assert parent == [EINVAL] * len(parent) and window == EINVAL, (what, form, n, parent, window)
            for n in (BIG, (1 << 64) - 1):                                    # nmetrics > 0xffffffff alone: LH_ERANGE
                parent, window = _both(L, fam, ids_form, dev, n=n, **good)
                assert parent == [ERANGE] and window == ERANGE, (form, n, parent, window)
            parent, window = _both(L, fam, ids_form, dev, n=0, **good)        # nmetrics == 0: LH_OK, no handle is looked at
            assert parent == [0] and window == 0, (form, parent, window)
    assert {"a NULL list", "NULL ids", "no output pointer at all", "flags 0x1", *(w.split(" by ")[0] for w in fam["bad_lead"])} <= seen
    assert all(np.all(a == 7) for a in arrays.values())                       # nothing was written, by either form
