"""Kept history of several processes brought into ONE name space (no GPU needed for the maps): every process of a fleet interns
its names in arrival order, a restarted process in another order than before, so row r of one handle and row r of another are
different names.  union_names builds, from the name lists of the handles' rows (Engine.metric_name per row, stored beside each blob
with loghisto_amd.keptfile.pack_names), the union and the map lh_kept_gather* takes; aggregate runs the gather."""
from __future__ import annotations

import numpy as np

NO_ROW = 0xffffffff                      # LH_KEPT_NO_ROW


def union_names(name_lists, firsts=None):
    """-> (union, src): `union` holds every name of the lists once, in order of first appearance (list by list, row by row); src
    is uint32[len(name_lists), len(union)] with src[i, j] = the ABSOLUTE row of union[j] in list i -- firsts[i] + its index there,
    firsts=None: every list starts at row 0 -- or NO_ROW where list i lacks the name.  A name twice in one list is a ValueError
    (a many-to-one roll-up within a handle is not a gather)."""
    lists = [list(names) for names in name_lists]
    firsts = [0] * len(lists) if firsts is None else [int(f) for f in firsts]
    if len(firsts) != len(lists):
        raise ValueError("one first per name list")
    at, union = {}, []
    for names in lists:
        if len(set(names)) != len(names):
            raise ValueError("a name appears twice in one list")
        for name in names:
            if name not in at:
                at[name] = len(union)
                union.append(name)
    src = np.full((len(lists), len(union)), NO_ROW, dtype=np.uint32)
    for i, (names, first) in enumerate(zip(lists, firsts)):
        if first < 0 or first + len(names) > NO_ROW:
            raise ValueError("rows are below 0xffffffff (the value is NO_ROW)")
        for r, name in enumerate(names):
            src[i, at[name]] = first + r
    return union, src


def aggregate(kepts, name_lists, stream=None):
    """-> (Kept, union): the handles `kepts`, whose rows carry the names name_lists[i] (from each handle's own first row on), summed
    per NAME into one new handle of rows [0, len(union)) in union_names' order -- Kept.gather over union_names' map.  At most
    loghisto_amd._native.MAX_KEPT handles a call: gather in groups over ONE union, then Kept.merge."""
    kepts = list(kepts)
    if not kepts or len(kepts) != len(name_lists):
        raise ValueError("one name list per handle, and at least one handle")
    for k, names in zip(kepts, name_lists):
        if len(names) > k.info["nrows"]:
            raise ValueError("more names than the handle has rows")
    union, src = union_names(name_lists, [k.info["first"] for k in kepts])
    return kepts[-1].gather(src, kepts[:-1], first=0, stream=stream), union
