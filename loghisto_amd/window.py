"""A rolling window of kept intervals whose total is advanced, not rebuilt (Kept.slide, lh_kept_slide): p99 over the last
minute, emitted every second, reads one handle of the window and the two that changed instead of all sixty.

    w = KeptWindow(60)
    every second:  old = w.push(snapshot.keep());  if old: old.close();  w.total.across((), [0.99])

The totals are exact: cells are unsigned 64-bit counts, so after any number of pushes w.total is byte for byte what
Kept.merge of w.handles gives.  No threads; the caller's handles stay the caller's.
"""
from __future__ import annotations

from collections import deque
from typing import Optional

import numpy as np

from . import _native as N
from .engine import Kept


def burn_fires(cum, total, budget, rate):
    """The burn-rate rule of Kept.burn / lh_kept_burn* in NumPy, for one window or several: with cum and total of shape (n,) or
    (nwin, n) -- the samples at or below each name's bound and all of its samples, as Kept.slo returns them for one bound a name --
    budget of shape (n,) and rate a scalar or of shape (nwin,):

        bad = total - cum;  t = rate * budget;  fires = total != 0 and float64(bad) > t * float64(total)

    in IEEE doubles, each product rounded once, the compare strict: a tie does not fire, a name without samples does not, and a NaN
    budget never does.  Returns the boolean array of cum's shape; a name is reported iff it fires in every window:
    burn_fires(...).all(axis=0).  This is the reference the device's decisions are held to, and what a user can recompute from
    Kept.burn(counts=True)."""
    cum, total = np.asarray(cum, dtype=np.uint64), np.asarray(total, dtype=np.uint64)
    rate = np.asarray(rate, dtype=np.float64)
    if rate.ndim == 1 and cum.ndim == 2:
        rate = rate[:, None]
    t = rate * np.asarray(budget, dtype=np.float64)
    bad = total - cum                                              # uint64: wraps as the device's does
    with np.errstate(invalid="ignore"):
        return (total != 0) & (bad.astype(np.float64) > t * total.astype(np.float64))


class KeptWindow:
    """The last `size` kept intervals and their running total."""

    def __init__(self, size: int):
        if size < 1:
            raise ValueError("a window holds at least one interval")
        self.size = size
        self.handles: deque = deque()          # the live intervals, the oldest first: the caller's
        self.total: Optional[Kept] = None      # their sum: the window's own, replaced by every push

    def push(self, kept: Kept) -> Optional[Kept]:
        """`kept` becomes the newest interval.  Returns the interval that left the window (the caller closes it), or None
        while the window fills.  After a KeptUnderflow or any other failure the window is as it was."""
        oldest = self.handles[0] if len(self.handles) == self.size else None
        if self.total is None:
            total = kept.slide()                                   # a copy: the window owns its total
        else:
            total = self.total.slide(add=[kept], sub=[oldest] if oldest else ())
            self.total.close()
        self.total = total
        self.handles.append(kept)
        return self.handles.popleft() if oldest else None

    def _newest_and_earlier(self):
        handles = list(self.handles)
        if not handles:
            raise ValueError("the window holds no interval yet")
        if len(handles) > N.MAX_KEPT:
            raise ValueError(f"a call reads at most {N.MAX_KEPT} handles; the window holds {len(handles)}")
        return handles[-1], handles[:-1]

    def series(self, percentiles, windows=None, nmetrics: Optional[int] = None, first: int = 0, ids=None, out=None, stream=None):
        """Kept.series over self.handles, the oldest first: `windows` are (lo, hi) positions among them, None: one per
        interval.  nmetrics / first / ids / out / stream as there.  ValueError above N.MAX_KEPT intervals."""
        newest, earlier = self._newest_and_earlier()
        return newest.series(percentiles, earlier, windows, nmetrics, first, ids, out, stream)

    def heat(self, bounds, windows=None, nmetrics: Optional[int] = None, first: int = 0, ids=None, out=None, stream=None):
        """Kept.heat over self.handles, the oldest first; as series()."""
        newest, earlier = self._newest_and_earlier()
        return newest.heat(bounds, earlier, windows, nmetrics, first, ids, out, stream)

    def slo(self, bounds, windows=None, nmetrics: Optional[int] = None, first: int = 0, ids=None, out=None, stream=None):
        """Kept.slo over self.handles, the oldest first: a row of bounds per name; as series()."""
        newest, earlier = self._newest_and_earlier()
        return newest.slo(bounds, earlier, windows, nmetrics, first, ids, out, stream)

    def burn(self, bounds, budget, rates, k: int, windows=None, nmetrics: Optional[int] = None, first: int = 0, ids=None,
             counts: bool = False, out=None, stream=None):
        """Kept.burn over self.handles, the oldest first: the names that burn their budget in every one of `windows`."""
        newest, earlier = self._newest_and_earlier()
        return newest.burn(bounds, budget, rates, k, earlier, windows, nmetrics, first, ids, counts, out, stream)

    def spread_series(self, percentiles, windows=None, nmetrics: Optional[int] = None, first: int = 0, ids=None, out=None,
                      stream=None):
        """Kept.spread_series over self.handles, the oldest first; as series()."""
        newest, earlier = self._newest_and_earlier()
        return newest.spread_series(percentiles, earlier, windows, nmetrics, first, ids, out, stream)

    def drift(self, windows=None, against=None, nmetrics: Optional[int] = None, first: int = 0, ids=None, out=None, stream=None):
        """Kept.drift over self.handles, the oldest first: `windows` are ((base_lo, base_hi), (cur_lo, cur_hi)) positions among
        them -- with against=(lo, hi), a fixed baseline, (cur_lo, cur_hi) only, None: one per interval --, None without
        `against`: each interval against the one before it.  The rest as series()."""
        newest, earlier = self._newest_and_earlier()
        return newest.drift(windows, earlier, against, nmetrics, first, ids, out, stream)

    def top_series(self, k: int, by: str = "count", arg: Optional[float] = None, ascending: bool = False, windows=None,
                   nmetrics: Optional[int] = None, first: Optional[int] = None, out=None, stream=None):
        """Kept.top_series over self.handles, the oldest first: the k leaders of each window, `windows` as for series()."""
        newest, earlier = self._newest_and_earlier()
        return newest.top_series(k, by, arg, ascending, earlier, windows, nmetrics, first, out, stream)

    def movers_series(self, k: int, by: str = "ks", arg: Optional[float] = None, ascending: bool = False, windows=None,
                      against=None, nmetrics: Optional[int] = None, first: Optional[int] = None, out=None, stream=None):
        """Kept.movers_series over self.handles, the oldest first: the k names that moved most in each window, `windows` /
        `against` as for drift()."""
        newest, earlier = self._newest_and_earlier()
        return newest.movers_series(k, by, arg, ascending, earlier, windows, against, nmetrics, first, out, stream)

    def close(self):
        """Releases what the window made, its total; the intervals pushed stay usable and are the caller's to close."""
        if self.total is not None:
            self.total.close()
            self.total = None
        self.handles.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
