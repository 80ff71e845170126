"""NumPy oracle of the tracker's split-and-merge stage on an unstructured mesh (split_and_merge_objects_parallel,
marEx/track.py:3804-4814, with partition_nn_unstructured_optimised, 5246-5353, partition_centroid_unstructured, 5357-5419,
and compute_id_time_dict, 2658-2728): the algorithm restated child by child on top of mesh_objects_oracle, with int64
fixed-point area sums and the float64 chord rule for the nearest centroid.  The nearest-neighbour partition
is the literal hop / parent / direction loop.  Imports nothing from marex_amd; not a test module."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_objects_oracle as mo  # noqa: E402

MAX_MERGES = 20    # merges per timestep and iteration (track.py:3828)
MAX_PARENTS = 10   # parents per merge (track.py:3829)
MAX_NEW_IDS = 255  # new IDs per timestep and iteration (updates_ids, track.py:3925)
I32_MAX = 2 ** 31 - 1


class OracleTrackingError(Exception):
    pass


class OracleConfigurationError(Exception):
    pass


def unit_vectors(lat_deg, lon_deg):
    """float64 [3, n]: the expressions of the weight tables (cos lat cos lon, cos lat sin lon, sin lat)."""
    lat_r = np.radians(np.asarray(lat_deg, dtype=np.float64).reshape(-1))
    lon_r = np.radians(np.asarray(lon_deg, dtype=np.float64).reshape(-1))
    cl = np.cos(lat_r)
    return np.stack([cl * np.cos(lon_r), cl * np.sin(lon_r), np.sin(lat_r)])


def nearest_centroid(u, pv):
    """Index of the first nearest column of pv [3, k] for every column of u [3, n]: smallest ((dx dx + dy dy) + dz dz)."""
    dx = u[0][:, None] - pv[0][None, :]
    dy = u[1][:, None] - pv[1][None, :]
    dz = u[2][:, None] - pv[2][None, :]
    return np.argmin((dx * dx + dy * dy) + dz * dz, axis=1)


def partition_centroid(child_mask, u, pv):
    """Owner index per cell of the mesh (255 outside the child): every child cell takes its nearest centroid."""
    owner = np.full(child_mask.size, 255, np.uint8)
    owner[child_mask] = nearest_centroid(u[:, child_mask], pv)
    return owner


def partition_nn(child_mask, owner, nbr0, max_hops, u, pv):
    """partition_nn_unstructured_optimised, literally.  ``owner`` uint8 [C]: parent index of the parents' cells in the
    previous slice, 255 = unclaimed.  Returns ``(owner, info)``; child cells still unclaimed take the nearest centroid."""
    owner = owner.copy()
    k = pv.shape[1]
    info = {"hops": 0, "leftover": 0, "capped": False, "early_stop": False, "nonchild_only_hop": False, "substeps_claiming": 0}
    hops = 0
    any_un = bool(np.any(child_mask & (owner == 255)))
    while hops < max_hops and any_un:
        hops += 1
        updates = claimed = False
        for p in range(k):
            for i in range(3):
                nb = nbr0[i, owner == p]
                nb = nb[nb >= 0]
                new = nb[owner[nb] == 255]
                if new.size:
                    claimed = True
                    info["substeps_claiming"] += 1
                owner[new] = p
                if np.any(child_mask[new]):
                    updates = True
        if not updates:
            info["early_stop"] = True
            info["nonchild_only_hop"] = claimed
            break
        any_un = bool(np.any(child_mask & (owner == 255)))
    left = child_mask & (owner == 255)
    info["hops"] = hops
    info["leftover"] = int(left.sum())
    info["capped"] = bool(hops == max_hops and any_un and not info["early_stop"])
    if left.any():
        owner[left] = nearest_centroid(u[:, left], pv)
    return owner, info


def hop_cap(parent_areas32, mean_cell_area):
    """track.py:4061-4072."""
    return max(int(np.sqrt(float(np.float64(np.max(parent_areas32)) / mean_cell_area)) * 2.0), 20) * 2


def chunk_ranges(chunks):
    out, s = [], 0
    for n in chunks:
        out.append((s, s + int(n)))
        s += int(n)
    return out


def _area32(q0, mask, e):
    return np.float32(float(int(q0[mask].sum(dtype=np.int64))) / 2.0 ** e)


def _fraction(ov32, a32, b32):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(ov32) / np.float64(min(a32, b32))


def _enforce_fractions(ov, pid, parea):
    """The fractions enforce_overlap_threshold compares with the threshold."""
    area = {int(i): np.float32(a) for i, a in zip(pid, parea)}
    return [float(_fraction(r[2], area[int(r[0])], area[int(r[1])])) for r in ov if int(r[0]) in area and int(r[1]) in area]


def split_and_merge(ids, q, e, nbr0, cell_areas, lat, lon, threshold, chunks, nn_partitioning, max_iteration=40):
    """Returns a dict: ``field`` int32 [T, C], ``props`` (ID, area, centroid), ``pairs`` int32 (n, 2), ``merges`` (list of
    ``(iteration, t, child_ids, parent_ids, areas)`` in order), ``events`` (the merge_events variables with ``merge_tidx`` in
    place of ``merge_time``), ``iterations``, ``fractions`` (every fraction compared with the threshold, start-up and final pair lists included) and
    ``nn`` (the info of every nearest-neighbour partition)."""
    field = np.asarray(ids).astype(np.int32).copy()
    T, C = field.shape
    q0 = q[0]
    nbr0 = np.asarray(nbr0)
    chunks = [int(c) for c in chunks]
    if sum(chunks) != T:
        raise OracleConfigurationError(f"chunks {chunks} do not cover {T} timesteps")
    if any(c == 1 for c in chunks):
        raise OracleConfigurationError("a time chunk of one step")
    timechunks = chunks[0]
    u = unit_vectors(lat, lon)
    mean_cell_area = float(np.asarray(cell_areas).astype(np.float32).mean())

    _, pid, _, parea, _ = mo.object_properties(field, q, e)
    ov_all = mo.find_overlapping_objects(field, q, e)
    ov = mo.enforce_overlap_threshold(ov_all, pid, parea, threshold)
    fractions = list(_enforce_fractions(ov_all, pid, parea))
    uc, cc = np.unique(ov[:, 1], return_counts=True) if len(ov) else (np.zeros(0), np.zeros(0, int))
    merging = set(int(v) for v in uc[cc > 1])
    counter = int(pid.max()) + 1 if pid.size else 1
    processed = set()
    merges, nn_info = [], []
    iteration = 0
    zeros = np.zeros(C, np.int32)

    while merging and iteration < max_iteration:
        per_t = {}
        for cid in sorted(merging):  # ascending ID: a READING (the reference iterates a Python set)
            rows = np.nonzero((field == cid).any(axis=1))[0]
            if rows.size:
                per_t.setdefault(int(rows[0]), []).append(cid)
        max_merges = max((len(v) for v in per_t.values()), default=0)
        bases = np.arange(T, dtype=np.int64) * max_merges * timechunks + counter
        if bases.max() > I32_MAX - MAX_NEW_IDS:
            raise OracleTrackingError("temporary IDs overflow int32")
        snap = field.copy()
        it_merges, final, drawn = [], [], {}
        for s, e_ in chunk_ranges(chunks):
            work = snap[s:e_].copy()
            queue = {t: list(per_t.get(t, [])) for t in range(s, e_)}
            chunk_final = []
            for t in range(s, e_):
                data_m1 = (snap[s - 1] if s > 0 else zeros) if t == s else work[t - 1 - s]
                data_t = work[t - s]
                data_p1 = (snap[e_] if e_ < T else zeros) if t == e_ - 1 else work[t + 1 - s]
                next_new = int(bases[t])
                n_merges = n_new = 0
                while queue[t]:
                    child = queue[t].pop(0)
                    child_mask = data_t == child
                    cand = np.unique(data_m1[child_mask])
                    parents, pareas, ovareas, pcen = [], [], [], []
                    for par in cand[cand > 0]:
                        if len(parents) >= MAX_PARENTS:
                            raise OracleTrackingError("Too many parent objects for tracking")
                        pmask = data_m1 == par
                        a0, a1 = _area32(q0, pmask, e), _area32(q0, child_mask, e)
                        ova = _area32(q0, pmask & child_mask, e)
                        fr = _fraction(ova, a0, a1)
                        fractions.append(float(fr))
                        if fr < threshold:
                            continue
                        S = np.array([[int(q[k][pmask].sum(dtype=np.int64))] for k in range(4)], dtype=np.int64)
                        _, cen = mo._finish(S, e)
                        parents.append(int(par))
                        pareas.append(a0)
                        ovareas.append(ova)
                        pcen.append(cen[:, 0])
                    if len(parents) < 2:
                        continue
                    n_par = len(parents)
                    child_ids = [child] + list(range(next_new, next_new + n_par - 1))
                    if n_merges >= MAX_MERGES:
                        raise OracleTrackingError("Too many merge operations")
                    if n_new + n_par - 1 > MAX_NEW_IDS:
                        raise OracleTrackingError("Too many new objects in one timestep")
                    n_merges += 1
                    n_new += n_par - 1
                    it_merges.append((t, child_ids, parents, ovareas))
                    drawn[t] = (int(bases[t]), next_new + n_par - 1)
                    pcen = np.array(pcen, dtype=np.float32)
                    pv = unit_vectors(pcen[:, 0], pcen[:, 1])
                    if nn_partitioning:
                        owner0 = np.full(C, 255, np.uint8)
                        for j, par in enumerate(parents):
                            owner0[data_m1 == par] = j
                        owner, info = partition_nn(child_mask, owner0, nbr0, hop_cap(np.array(pareas, np.float32), mean_cell_area),
                                                   u, pv)
                        info.update(t=t, child=child, iteration=iteration, cells=int(child_mask.sum()), parents=n_par)
                        nn_info.append(info)
                    else:
                        owner = partition_centroid(child_mask, u, pv)
                    data_t[child_mask] = np.array(child_ids, np.int32)[owner[child_mask]]
                    next_new += n_par - 1
                    found = []
                    for new_id in child_ids:
                        pm = data_t == new_id
                        if not pm.any():
                            continue
                        a0 = _area32(q0, pm, e)
                        cands = np.unique(data_p1[pm])
                        for pc in cands[cands > 0]:
                            cm = data_p1 == pc
                            fr = _fraction(_area32(q0, pm & cm, e), a0, _area32(q0, cm, e))
                            fractions.append(float(fr))
                            if fr > threshold:
                                found.append(int(pc))
                    if t < e_ - 1:
                        for c in found:
                            if c not in queue[t + 1]:
                                queue[t + 1].append(c)
                    else:
                        for c in found:
                            if c not in chunk_final:
                                if len(chunk_final) >= MAX_MERGES:
                                    raise OracleTrackingError("Excessive merge operations detected")
                                chunk_final.append(c)
            field[s:e_] = work
            final.extend(chunk_final)
        ranges = sorted(drawn.values())
        for (b0, n0), (b1, _) in zip(ranges[:-1], ranges[1:]):
            if n0 > b1:
                raise OracleTrackingError("Temporary IDs of two timesteps collide")
        temp = sorted({c for _, ch, _, _ in it_merges for c in ch if c >= counter})
        lookup = {tid: counter + k for k, tid in enumerate(temp)}
        if temp and max(n for _, n in ranges) - 1 > I32_MAX:
            raise OracleTrackingError("temporary IDs overflow int32")
        if lookup:
            keys = np.array(temp, np.int64)
            vals = np.array([lookup[k] for k in temp], np.int32)
            pos = np.clip(np.searchsorted(keys, field), 0, keys.size - 1)
            hit = keys[pos] == field
            field = np.where(hit, vals[pos], field).astype(np.int32)
        counter += len(temp)
        for t, ch, pa, ar in it_merges:
            merges.append((iteration, t, [lookup.get(c, c) for c in ch], [lookup.get(p, p) for p in pa], ar))
        final_mapped = set(lookup.get(c, c) for c in final)
        merging = final_mapped - processed
        processed |= final_mapped
        iteration += 1
    if iteration == max_iteration:
        raise OracleTrackingError("Maximum iterations reached in tracking algorithm")

    _, pid, _, parea, pcen = mo.object_properties(field, q, e)
    ov_all = mo.find_overlapping_objects(field, q, e)
    fractions.extend(_enforce_fractions(ov_all, pid, parea))
    pairs = mo.enforce_overlap_threshold(ov_all, pid, parea, threshold)[:, :2].astype(np.int32)
    return {"field": field, "props": {"ID": pid, "area": parea, "centroid": pcen}, "pairs": pairs, "merges": merges,
            "events": merge_events(merges), "iterations": iteration, "fractions": np.array(fractions), "nn": nn_info}


def merge_events(merges):
    """The variables of the reference's merge_events dataset (track.py:4751-4796); ``merge_tidx`` indexes the time axis."""
    mp = max((len(m[3]) for m in merges), default=1)
    mc = max((len(m[2]) for m in merges), default=1)
    P = np.full((len(merges), mp), -1, np.int32)
    Cc = np.full((len(merges), mc), -1, np.int32)
    A = np.full((len(merges), mp), -1, np.float32)
    for i, (_, _, ch, pa, ar) in enumerate(merges):
        P[i, :len(pa)], Cc[i, :len(ch)], A[i, :len(ar)] = pa, ch, ar
    return {"parent_IDs": P, "child_IDs": Cc, "overlap_areas": A, "merge_tidx": np.array([m[1] for m in merges], np.int64),
            "n_parents": np.array([len(m[3]) for m in merges], np.int8),
            "n_children": np.array([len(m[2]) for m in merges], np.int8)}


def count_events(pairs, ids):
    """Connected components of the pairs over the IDs."""
    ids = [int(i) for i in ids]
    root = {i: i for i in ids}

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a

    for a, b in np.asarray(pairs).tolist():
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            root[max(ra, rb)] = min(ra, rb)
    return len({find(i) for i in ids})
