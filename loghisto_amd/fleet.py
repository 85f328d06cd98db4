"""Kept history of several processes brought into ONE name space (no GPU needed for the maps): every process of a fleet interns
its names in arrival order, a restarted process in another order than before, so row r of one handle and row r of another are
different names.  union_names builds, from the name lists of the handles' rows (Engine.metric_name per row, stored beside each blob
with loghisto_amd.keptfile.pack_names), the union and the map lh_kept_gather* takes; aggregate runs the gather.
Rolling a handle up ACROSS names -- a service over its endpoints -- is lh_kept_group*: group_names builds its groups from the names'
labels, roll_up runs it."""
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


def group_names(names, key, first: int = 0):
    """-> (labels, goff, members): the CSR lh_kept_group* takes for a roll-up of the rows [first, first + len(names)) by label.
    key(name) is the label of a name, None to drop the name, or a tuple or list of labels for a name that feeds several groups
    (its service, and "everything").  `labels` stand in order of first appearance; group g = members[goff[g]:goff[g + 1]] holds
    the ABSOLUTE rows of the names with labels[g], in row order (a label a name gives twice counts it twice).  goff is uint64,
    members uint32."""
    names = list(names)
    if first < 0 or first + len(names) > NO_ROW:
        raise ValueError("rows are below 0xffffffff (the value is NO_ROW)")
    at, labels, rows = {}, [], []
    for r, name in enumerate(names):
        got = key(name)
        if got is None:
            continue
        for label in got if isinstance(got, (tuple, list)) else (got,):
            if label not in at:
                at[label] = len(labels)
                labels.append(label)
                rows.append([])
            rows[at[label]].append(first + r)
    goff = np.cumsum([0] + [len(x) for x in rows]).astype(np.uint64)
    members = np.array([r for x in rows for r in x], dtype=np.uint32)
    return labels, goff, members


def roll_up(kepts, names, key, stream=None):
    """-> (Kept, labels): the handles `kepts`, whose rows ALL carry the names `names` (from the last handle's first row on), summed
    per label of group_names(names, key) into one new handle of rows [0, len(labels)) -- Kept.group.  At most
    loghisto_amd._native.MAX_KEPT handles a call; a group may be as large as it likes."""
    kepts = list(kepts)
    if not kepts:
        raise ValueError("at least one handle")
    labels, goff, members = group_names(names, key, kepts[-1].info["first"])
    if not labels:
        raise ValueError("no name has a label")
    return kepts[-1].group((goff, members), kepts[:-1], first=0, stream=stream), labels
