"""An independent statement of the two integer steps that start a reconstruction, written from the text of cv-sfm
(cv-sfm/src/lib.rs:377-500, 992-999, 1190-1246, 1421) and from the contract text of include/akz.h in dicts, lists and numpy.  It
shares no code with include/akz_bootstrap_table_math.h, with the kernels or with cv_amd.three_view.join_pairs; the tests hold the
host build of the header to it in every byte, and it to join_pairs.

  shuffle_keys, shuffle_permutation   RS_BATCH_SHUFFLE's rule for the common matches
  join_lists                          the HashMap join of init_reconstruction on two inlier pair lists
  join                                rs_join_pairs_batch_device: verdicts, the gathered lists, the three output lists
  add_reconstruction                  rs_add_reconstruction_batch_device: acceptance, add_view three times, every output array

The output arrays start from the caller's fill (`out`, a dict of arrays): what the contract leaves unwritten stays as it was.
"""
import numpy as np

M64 = (1 << 64) - 1
NONE = 0xFFFFFFFF
JP_OK, JP_NO_MODEL, JP_FEW_INLIERS, JP_BAD_INDEX = range(4)
AR_OK, AR_NOT_ACCEPTED, AR_BAD_INDEX, AR_TAKEN, AR_BAD_TABLE = range(5)
TV_OK, TVC_OK, NOT_RECORDED = 0, 0, 16


def _mix(x):
    """splitmix64(x): the first output of the generator started at x"""
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def shuffle_keys(seed, scene, n):
    seed_s = (seed + 0x9E3779B97F4A7C15 * scene) & M64
    return [_mix(((seed_s ^ 0x5851F42D4C957F2D) + 0xD1342543DE82EF95 * j) & M64) >> 32 for j in range(n)]


def order_of(keys, stable=True):
    """position j holds the element with the j-th smallest key, ties in index order (`stable=False`: a deliberately broken rule,
    ties in descending index order)"""
    return sorted(range(len(keys)), key=lambda j: (keys[j], j if stable else -j))


def shuffle_permutation(seed, scene, n):
    return order_of(shuffle_keys(seed, scene, n))


def join_lists(first, second, last_wins=True):
    """lib.rs:992-998, 1190-1191, 1216, 1234 on two lists of (centre, other): the common matches in the order of `first`, the
    matches of one list whose centre feature the other lacks in the order of their own list.  A HashMap collected from a list
    keeps the LAST entry of a key (`last_wins=False`: a deliberately broken rule)."""
    def collect(pairs):
        m = {}
        for c, o in pairs:
            if last_wins or c not in m:
                m[c] = o
        return m
    in_first, in_second = collect(first), collect(second)
    triples = [(c, f, in_second[c]) for c, f in first if c in in_second]
    first_only = [(c, f) for c, f in first if c not in in_second]
    second_only = [(c, s) for c, s in second if c not in in_first]
    return triples, first_only, second_only


def gathered(pairs, npairs, inliers, n_inliers, cap):
    """the pair list of one slot in inlier order, or None where something lies outside"""
    if n_inliers > cap or npairs > cap:
        return None
    out = []
    for i in range(n_inliers):
        k = int(inliers[i])
        if k >= npairs:
            return None
        c, o = int(pairs[k][0]), int(pairs[k][1])
        if c >= cap or o >= cap:
            return None
        out.append((c, o))
    return out


def join(inp, out):
    """rs_join_pairs_batch_device on the arrays of checker.join_inputs -> `out` (checker.join_outputs' fill) written."""
    cap, shuffle = inp["cap"], inp["flags"] & 1
    for s in range(inp["n_scenes"]):
        a, b = int(inp["slot_first"][s]), int(inp["slot_second"][s])
        out["pose_first"][s], out["pose_second"][s] = inp["pose"][a], inp["pose"][b]
        lists = [gathered(inp["pairs"][k], int(inp["npairs"][k]), inp["inliers"][k], int(inp["n_inliers"][k]), cap) for k in (a, b)]
        counts_bad = any(int(inp[name][k]) > cap for name in ("npairs", "n_inliers") for k in (a, b))
        if NONE in (int(inp["best_id"][a]), int(inp["best_id"][b])):
            v = JP_NO_MODEL
        elif counts_bad:
            v = JP_BAD_INDEX
        elif min(int(inp["n_inliers"][a]), int(inp["n_inliers"][b])) < inp["minimum"]:
            v = JP_FEW_INLIERS
        elif None in lists:
            v = JP_BAD_INDEX
        else:
            v = JP_OK
        out["verdict"][s] = v
        out["ntriples"][s] = out["nfirst"][s] = out["nsecond"][s] = 0
        if v != JP_OK:
            continue
        triples, first_only, second_only = join_lists(*lists)
        if shuffle:
            triples = [triples[j] for j in shuffle_permutation(inp["seed"], s, len(triples))]
        for name, count, rows in (("triples", "ntriples", triples), ("first_only", "nfirst", first_only), ("second_only", "nsecond", second_only)):
            out[count][s] = len(rows)
            if rows:
                out[name][s, :len(rows)] = np.array(rows, np.uint32)
    return out


def _ascends(start, lo_ok, last):
    return all(int(start[i]) <= int(start[i + 1]) for i in range(len(start) - 1)) and lo_ok(int(start[-1]), last)


def add_reconstruction(inp, out, second_before_first=False):
    """rs_add_reconstruction_batch_device on the arrays of checker.add_inputs -> `out` (checker.add_outputs' fill) written.
    `second_before_first`: a deliberately broken rule — the second view's own rows in front of the first's."""
    cap, n_scenes, base, n_lm, n_obs, n_recons = inp["cap"], inp["n_scenes"], inp["view_base"], inp["n_landmarks"], inp["n_obs"], inp["n_recons"]
    start = inp["obs_start"] if inp["obs_start"] is not None else np.zeros(1, np.uint32)
    obs = inp["obs"] if inp["obs"] is not None else np.zeros((0, 2), np.uint32)
    bad = not _ascends(start[:n_lm + 1], lambda e, last: e <= last, n_obs)
    if n_recons:
        bad = bad or not _ascends(inp["recon_start"], lambda e, last: e == last, n_lm)
        bad = bad or not _ascends(inp["view_start"], lambda e, last: e == last, base)
    # the old table, unchanged
    landmarks = np.full((inp["n_blocks"], cap), NONE, np.uint32)
    rows = [[(int(b), int(f)) for b, f in obs[int(start[l]):int(start[l + 1])]] for l in range(n_lm)] if not bad else None
    old_rows_end = int(inp["recon_start"][-1]) if n_recons else n_lm
    old_views_end = int(inp["view_start"][-1]) if n_recons else base
    recon_start = [int(v) for v in inp["recon_start"][:n_recons]] if n_recons else []
    view_start = [int(v) for v in inp["view_start"][:n_recons]] if n_recons else []
    taken, accepted_n = set(), 0
    for s in range(n_scenes):
        blocks = [int(inp[name][s]) for name in ("ic", "i_first", "i_second")]
        counts = [int(inp["counts"][b]) for b in blocks]
        lists = [int(inp[name][s]) for name in ("ntriples", "nfirst", "nsecond")]
        views = [base + 3 * s + k for k in range(3)]
        out["views_out"][s] = views
        st = [0, 0, 0, 0]
        if bad or int(inp["tv_verdict"][s]) != TV_OK or (inp["skip"] is not None and int(inp["skip"][s]) != 0):
            v = AR_NOT_ACCEPTED
        elif len(set(blocks)) != 3 or max(counts + lists) > cap:
            v = AR_BAD_INDEX
        else:
            # the accepted matches: (centre, first or None, second or None)
            matches = [(int(c), int(f), int(g)) for (c, f, g), ok in zip(inp["triples"][s][:lists[0]], inp["combined"][s]) if ok]
            st[0] = len(matches)
            more = [(int(c), int(f), None) for (c, f), ok in zip(inp["first_only"][s][:lists[1]], inp["first_ok"][s]) if ok]
            st[1] = len(more)
            matches += more
            more = [(int(c), None, int(g)) for (c, g), ok in zip(inp["second_only"][s][:lists[2]], inp["second_ok"][s]) if ok]
            st[2] = len(more)
            matches += more
            named = [[m[k] for m in matches if m[k] is not None] for k in range(3)]
            in_range = all(x < counts[k] for k in range(3) for x in named[k])
            once = all(len(set(named[k])) == len(named[k]) for k in range(3))
            v = AR_OK if in_range and once else AR_BAD_INDEX
            if v == AR_OK and taken & set(blocks):
                v = AR_TAKEN
        out["frame_verdict"][s] = v
        out["constraint_verdict_out"][s] = TVC_OK if v == AR_OK else NOT_RECORDED
        recon_start.append(old_rows_end if bad else len(rows))
        view_start.append(old_views_end if bad else views[0])
        if v != AR_OK:
            out["stats"][s] = 0
            continue
        taken |= set(blocks)
        accepted_n += 1
        # add_view three times (lib.rs:432-500): the centre view makes a landmark of every feature; a later view's feature
        # joins the landmark its accepted match names, any other becomes a landmark of its own
        of_centre = {}
        for j in range(counts[0]):
            of_centre[j] = len(rows)
            rows.append([(views[0], j)])
        own = {1: [], 2: []}
        for k in (1, 2):
            to_centre = {m[k]: m[0] for m in matches if m[k] is not None}
            for j in range(counts[k]):
                if j in to_centre:
                    rows[of_centre[to_centre[j]]].append((views[k], j))
                else:
                    own[k].append([(views[k], j)])
        rows += (own[2] + own[1]) if second_before_first else (own[1] + own[2])
        st[3] = counts[0] + len(own[1]) + len(own[2])
        out["stats"][s] = st
        for k in range(3):
            out["kps_dst"][views[k]] = inp["kps"][blocks[k]]
            out["counts_dst"][views[k]] = counts[k]
        out["poses"][views[0]] = np.eye(3, 4).reshape(12)
        out["poses"][views[1]], out["poses"][views[2]] = inp["pose_out"][s][:12], inp["pose_out"][s][12:]
        out["constraint_poses_out"][s] = inp["pose_out"][s]
    # the table
    if bad:
        out["obs_start_out"][:n_lm + 1] = start[:n_lm + 1]
        out["obs_start_out"][n_lm + 1:] = start[n_lm]
        for l in range(n_lm):
            out["obs_counts_out"][l] = int(start[l + 1]) - int(start[l]) if int(start[l + 1]) >= int(start[l]) else 0
        out["obs_counts_out"][n_lm:inp["lm_room"]] = 0
        out["obs_out"][:n_obs] = obs[:n_obs]
        n_rows, total = n_lm, n_obs
    else:
        at = int(start[0])                                   # (a table need not begin at 0: what lies in front is copied too)
        out["obs_out"][:at] = obs[:at]
        for r, row in enumerate(rows):
            out["obs_start_out"][r] = at
            out["obs_counts_out"][r] = len(row)
            for b, f in row:
                out["obs_out"][at] = (b, f)
                if b < inp["n_blocks"] and f < cap:
                    landmarks[b, f] = min(int(landmarks[b, f]), r)
                at += 1
        n_rows, total = len(rows), at
        out["obs_start_out"][n_rows:] = total
        out["obs_counts_out"][n_rows:inp["lm_room"]] = 0
    out["landmarks_out"][:] = landmarks
    out["recon_start_out"][:] = recon_start + [old_rows_end if bad else n_rows]
    out["view_start_out"][:] = view_start + [old_views_end if bad else base + 3 * n_scenes]
    out["counts_out"][:] = (n_rows, total, n_recons + n_scenes, accepted_n)
    out["call_verdict"][0] = AR_BAD_TABLE if bad else AR_OK
    return out
