"""An independent statement of cv-sfm's loop closure between two reconstructions and of its normalisation, in dicts, sets,
lists and numpy, written from the reference's text and not from include/akz_reconstruction_merge_math.h:

  the landmark map of try_merge_reconstructions     cv-sfm/src/lib.rs:2159-2170
  incorporate_reconstruction                        cv-sfm/src/lib.rs:1817-1887
  normalize_reconstruction                          cv-sfm/src/lib.rs:2241-2283
  WorldToWorld::from_camera_poses                   cv-core/src/pose.rs:322-324

A Reconstruction has `views` {block: View(pose 4x4, landmarks [key per feature, None for none])} and `landmarks` {key:
{block: feature}}.  Where the project departs from the reference (the order of a row and of the new keys, the
rule for a map that is not one-to-one, stable keys, the refusals) the departure is stated here in the same plain terms."""
from collections import Counter

import numpy as np

NONE = 0xFFFFFFFF
OK, BAD_TABLE, BAD_INDEX, SHARED_BLOCK = range(4)
NR_OK, NR_NOT_NORMAL, NR_BAD_INDEX = range(3)


class View:
    def __init__(self, pose, landmarks):
        self.pose, self.landmarks = pose, landmarks


class Reconstruction:
    """views {block: View}, landmarks {key: {block: feature}} from the rows of a table (row = key; an empty row is a
    tombstone) and the poses [n_blocks][12]"""

    def __init__(self, rows, poses, cap):
        self.landmarks = {key: dict(row) for key, row in enumerate(rows)}
        self.order = {key: [tuple(o) for o in row] for key, row in enumerate(rows)}
        self.views = {}
        for key, row in enumerate(rows):
            for block, feature in row:
                if block not in self.views:
                    pose = pose4(poses[block]) if block < len(poses) else None
                    self.views[block] = View(pose, [None] * cap)
                if feature < cap and self.views[block].landmarks[feature] is None:
                    self.views[block].landmarks[feature] = key


def pose4(p12):
    m = np.eye(4)
    m[:3] = np.asarray(p12, np.float64).reshape(3, 4)
    return m


def merge_map(matches, src_view_landmarks):
    """lib.rs:2159-2170: matches {feature: [dest landmarks]} of the bridging frame, the landmarks of its view in the source ->
    [(source landmark, dest_landmarks[0])] in ascending feature order; a feature without a source landmark gives nothing."""
    return [(src_view_landmarks[f], dests[0]) for f, dests in sorted(matches.items()) if src_view_landmarks[f] is not None]


def incorporate(dst_rows, src_rows, pairs, src_blocks, bridge_block, src_pose, poses, cap, n_blocks, skip=None):
    """incorporate_reconstruction on the rows of two tables.  -> dict(verdict, rows, counts, landmarks {(block, feature): key},
    src_key [per source landmark], poses [n_blocks][12])"""
    poses = np.array(poses, np.float64).reshape(n_blocks, 12)
    skip = [0] * len(src_blocks) if skip is None else list(skip)
    dst, src = Reconstruction(dst_rows, poses, cap), Reconstruction(src_rows, poses, cap)
    # the reference removes the bridging frame's view from the source before it incorporates (lib.rs:2176-2178); a view the
    # caller skips stands for one whose record was refused (lib.rs:1880-1884)
    src_views = [b for b, s in zip(src_blocks, skip) if not s and b != bridge_block]
    kept = [(b, f) for row in src_rows for b, f in row if b in set(src_views)]
    unchanged = dict(rows=[list(map(tuple, r)) for r in dst_rows], src_key=[NONE] * len(src_rows), poses=poses,
                     counts=[len(dst_rows), sum(len(r) for r in dst_rows), 0, 0, 0, 0])
    unchanged["landmarks"] = inverse(unchanged["rows"])
    if any(f >= cap for _, f in kept):
        return dict(unchanged, verdict=BAD_INDEX)
    if {b for b, _ in kept} & set(dst.views):                    # a frame has one view
        return dict(unchanged, verdict=SHARED_BLOCK)
    # the map: an entry counts iff nothing else names its source landmark and nothing else its destination landmark (the
    # reference's HashMap would keep the last of them and overwrite observations)
    n_src, n_dst = len(src_rows), len(dst_rows)
    cs = Counter(s for s, _ in pairs if s < n_src)
    cd = Counter(d for _, d in pairs if d < n_dst)
    landmark_map = {s: d for s, d in pairs if s < n_src and d < n_dst and cs[s] == 1 and cd[d] == 1}
    applied = len(landmark_map)
    # lib.rs:1830-1878: every feature of every source view goes to the landmark its source landmark is mapped to, or founds one
    members = {}
    for block in src_views:
        view = src.views.get(block)
        if view is None:
            continue
        for feature, src_landmark in enumerate(view.landmarks):
            if src_landmark is None:
                continue
            members.setdefault(src_landmark, []).append((block, feature))
    rows = [list(map(tuple, r)) for r in dst_rows]
    src_key = [NONE] * n_src
    for s in sorted(members):                                    # new keys ascend with the source key
        obs = sorted(members[s], key=src.order[s].index)         # a row keeps the source's order
        if s in landmark_map:
            rows[landmark_map[s]] += obs
        else:
            src_key[s] = len(rows)
            rows.append(obs)
    for s, d in landmark_map.items():
        src_key[s] = d
    # lib.rs:1824, 1835-1837 with pose.rs:322-324
    dest_to_src = np.linalg.inv(pose4(src_pose)) @ pose4(poses[bridge_block])
    out = poses.copy()
    for block in src_views:
        out[block] = (pose4(poses[block]) @ dest_to_src)[:3].reshape(12)
    total_src = sum(len(r) for r in src_rows)
    return dict(verdict=OK, rows=rows, src_key=src_key, poses=out, landmarks=inverse(rows),
                counts=[len(rows), sum(len(r) for r in rows), applied, len(pairs) - applied, len(rows) - n_dst, total_src - len(kept)])


def inverse(rows):
    """{(block, feature): the lowest key whose row lists it}"""
    inv = {}
    for key, row in enumerate(rows):
        for o in row:
            inv.setdefault(tuple(o), key)
    return inv


def normalize(view_blocks, counts, landmarks, world, poses, constraint_poses, cap, n_blocks):
    """normalize_reconstruction: landmarks [n_blocks][cap] keys (NONE for none), world [n][4] (w < 0: no robust point), poses
    [n_blocks][12], constraint_poses [n][2][12].  -> dict(verdict, mean, count, poses, constraint_poses)"""
    poses = np.array(poses, np.float64).reshape(n_blocks, 12)
    cposes = np.array(constraint_poses, np.float64).reshape(-1, 2, 12)
    out = dict(verdict=NR_BAD_INDEX, mean=0.0, count=0, poses=poses, constraint_poses=cposes)
    if any(b >= n_blocks for b in view_blocks) or counts[view_blocks[0]] > cap:
        return out
    first = pose4(poses[view_blocks[0]])
    distances = []
    for feature in range(int(counts[view_blocks[0]])):
        landmark = int(landmarks[view_blocks[0]][feature])
        if landmark >= len(world) or world[landmark][3] < 0:     # no landmark, or triangulate_landmark_robust gave None
            continue
        camera = first @ np.asarray(world[landmark], np.float64)
        if camera[3] == 0:                                       # Projective::point() is None
            continue
        distances.append(float(np.linalg.norm(camera[:3] / camera[3])))
    mean = float(np.mean(distances)) if distances else 0.0
    out.update(mean=mean, count=len(distances), verdict=NR_NOT_NORMAL)
    if not (np.isfinite(mean) and abs(mean) >= np.finfo(np.float64).tiny):
        return out
    factor, transform = 1.0 / mean, np.linalg.inv(first)
    new = poses.copy()
    for block in view_blocks:
        m = pose4(poses[block]) @ transform
        m[:3, 3] *= factor
        new[block] = m[:3].reshape(12)
    cnew = cposes.copy().reshape(-1, 3, 4)
    cnew[:, :, 3] *= factor
    return dict(verdict=NR_OK, mean=mean, count=len(distances), poses=new, constraint_poses=cnew.reshape(-1, 2, 12))
