"""An independent statement of the covisibility search, the record and the rows in plain Python dicts, sets and lists, written
from the reference's text (cv-sfm/src/lib.rs:2438-2556, 1939-1990, 2092-2109, 2519-2532, 167-180) with the orders DESIGN.md §7
documents: candidates ascending by block, pairs lexicographic, stable sorts, a seeded mix in place of the shuffle.  It shares no
code with include/akz_covisibility_math.h."""
import itertools

MAX_CANDIDATE_VIEWS = 128
OK, FEW_CONSTRAINTS, BAD_INDEX, NO_GRAPH = range(4)
NOT_RECORDED = 16
F_CAPPED, F_LIMIT = 1, 2
M32 = 0xFFFFFFFF


def settings(min_cov=16, max_constraints=64, min_new=4, min_lm=24, max_lm=64, limit=0, seed=0):
    """the reference's defaults (cv-sfm/src/settings.rs:453-475)"""
    return dict(min_cov=min_cov, max_constraints=max_constraints, min_new=min_new, min_lm=min_lm, max_lm=max_lm,
                limit=limit or max_constraints, seed=seed)


def mix(seed, landmark):
    """MurmurHash3's 32-bit finaliser over seed ^ landmark * 0x9E3779B9"""
    h = (seed ^ (landmark * 0x9E3779B9)) & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def _table(start, obs, n_blocks, cap):
    """-> (broken start array?, per landmark: dict view -> first feature, list length, names something outside?;
    dict (view, feature) -> the lowest landmark naming it)"""
    n_obs = len(obs)
    broken, lms, owner = False, [], {}
    for l in range(len(start) - 1):
        s, e = int(start[l]), int(start[l + 1])
        if s > e or e > n_obs:
            broken = True
            lms.append(({}, 0, True))
            continue
        views, bad = {}, False
        for b, f in obs[s:e]:
            b, f = int(b), int(f)
            if b >= n_blocks or f >= cap:
                bad = True
                continue
            views.setdefault(b, f)
            owner[(b, f)] = min(owner.get((b, f), l), l)
        lms.append((views, e - s, bad))
    return broken, lms, owner


def candidates(start, obs, reason, targets, n_blocks, cap, p):
    """-> dict(views, lm_start, lm, slot_count, verdict, stats, detail); detail[t] = dict(triples, unique, emitted) for the
    tests that must not be vacuous"""
    broken, lms, owner = _table(start, obs, n_blocks, cap)
    limit, min_cov = p["limit"], max(p["min_cov"], 1)
    views_out, counts, lists, verdicts, stats, detail = [], [], [], [], [], []
    for v in targets:
        v = int(v)
        mine = [(j, owner[(v, j)]) for j in range(cap) if (v, j) in owner] if v < n_blocks else []
        if v >= n_blocks or broken or any(lms[l][2] for _, l in mine):
            views_out += [(0, 0, 0)] * limit
            counts += [0] * limit
            lists += [[] for _ in range(limit)]
            verdicts.append(BAD_INDEX)
            stats.append([0] * 8)
            detail.append(dict(triples=[], unique=[], emitted=[]))
            continue
        robust = [(j, l) for j, l in mine if reason[l] == 0]
        covis = {}
        for j, l in robust:                                              # lib.rs:2541-2553
            for coview in lms[l][0]:
                if coview != v:
                    covis.setdefault(coview, []).append((j, l))
        covis = {u: ls for u, ls in covis.items() if len(ls) >= min_cov}   # lib.rs:2446-2451
        capped = len(covis) > MAX_CANDIDATE_VIEWS
        if capped:
            keep = sorted(covis, key=lambda u: (-len(covis[u]), u))[:MAX_CANDIDATE_VIEWS]
            covis = {u: covis[u] for u in keep}
        triples = []
        for a, b in itertools.combinations(sorted(covis), 2):            # lib.rs:2463-2481
            both = [(j, l) for j, l in covis[a] if b in lms[l][0]]
            if len(both) >= min_cov:
                triples.append((tuple(sorted((v, a, b))), both))
        triples.sort(key=lambda t: -len(t[1]))                           # lib.rs:2484-2486, stable
        visited, unique = set(), []
        for i, (tv, _) in enumerate(triples):                            # lib.rs:2490-2495
            if len(unique) == p["max_constraints"]:
                break
            for x in tv:                                                 # any(): stops at the first insert that succeeds
                if x not in visited:
                    visited.add(x)
                    unique.append(i)
                    break
        taken = set(unique)
        chain = unique + [i for i in range(len(triples)) if i not in taken]   # lib.rs:2499-2510
        alive = [i for i in chain if len(triples[i][1]) >= p["min_lm"]]       # lib.rs:1949
        emitted = alive[:limit]
        for i in emitted:
            tv, both = triples[i]
            keyed = sorted(range(len(both)), key=lambda k: (-min(len(lms[both[k][1]][0]), 0x7FFFF),
                                                            mix(p["seed"], both[k][1]) if p["seed"] else 0, k))
            rows = []
            for k in keyed[:p["max_lm"]]:
                j, l = both[k]
                rows.append(tuple(j if x == v else lms[l][0][x] for x in tv))
            views_out.append(tv)
            counts.append(len(both))
            lists.append(rows)
        pad = limit - len(emitted)
        views_out += [(0, 0, 0)] * pad
        counts += [0] * pad
        lists += [[] for _ in range(pad)]
        verdicts.append(OK)
        stats.append([len(robust), len(covis), len(triples), len(unique), len(emitted),
                      (F_CAPPED if capped else 0) | (F_LIMIT if len(alive) > limit else 0), 0, 0])
        detail.append(dict(triples=triples, unique=unique, emitted=emitted))
    lm_start, lm = [0], []
    for rows in lists:
        lm += rows
        lm_start.append(len(lm))
    return dict(views=views_out, lm_start=lm_start, lm=lm, slot_count=counts, verdict=verdicts, stats=stats, detail=detail)


def record(constraint_verdict, targets, target_verdict, graph_start, p):
    """-> (recorded [n_slots], verdict [n_targets], recorded counts [n_targets])"""
    limit = p["limit"]
    recorded, verdicts, ns = [], [], []
    for t, v in enumerate(targets):
        v = int(v)
        mine = [int(x) for x in constraint_verdict[t * limit:(t + 1) * limit]]
        refused = [x if x else NOT_RECORDED for x in mine]
        if target_verdict[t] == BAD_INDEX:
            recorded += refused
            verdicts.append(BAD_INDEX)
            ns.append(0)
            continue
        sizes = [int(graph_start[g + 1]) - int(graph_start[g]) for g in range(len(graph_start) - 1)
                 if int(graph_start[g]) <= v < int(graph_start[g + 1])]
        if not sizes:
            recorded += refused
            verdicts.append(NO_GRAPH)
            ns.append(0)
            continue
        out, n = [], 0
        for x in mine:                                                   # .filter_map(..).take(..), lib.rs:2511-2514
            if x == 0 and n < p["max_constraints"]:
                out.append(0)
                n += 1
            else:
                out.append(x if x else NOT_RECORDED)
        if n < p["min_new"] and n + 1 < sizes[0]:                        # lib.rs:2098-2102
            recorded += refused
            verdicts.append(FEW_CONSTRAINTS)
            ns.append(0)
        else:
            recorded += out
            verdicts.append(OK)
            ns.append(n)
    return recorded, verdicts, ns


def rows(views, n_views):
    """-> (row_start, row_edges, flag): view v's row holds 6 c + s for every edge slot s of constraint c whose target is v
    (targets of the six slots: views {0, 0, 1, 1, 2, 2} of the triple, lib.rs:167-180), ascending"""
    table = {v: [] for v in range(n_views)}
    flag = 0
    for c, tv in enumerate(views):
        if any(int(x) >= n_views for x in tv):
            flag = 1
            continue
        for s, k in enumerate((0, 0, 1, 1, 2, 2)):
            table[int(tv[k])].append(6 * c + s)
    row_start, row_edges = [0], []
    for v in range(n_views):
        row_edges += sorted(table[v])
        row_start.append(len(row_edges))
    return row_start, row_edges, flag
