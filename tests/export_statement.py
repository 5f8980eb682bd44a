"""An independent statement of cv-sfm's export of a reconstruction, in dicts, lists and numpy, written from the reference's
text and not from include/akz_export_math.h:

  VSlam::export_reconstruction        cv-sfm/src/lib.rs:2285-2340
  export (vertices, faces, the file)  cv-sfm/src/export.rs

A reconstruction is `world` [n][4] (row = landmark key; w < 0: triangulate_landmark_robust gave None), `rows` (per landmark its
observations [(block, feature)], an empty one a tombstone), `colors` {(block, feature): (r, g, b)} as a [n_blocks][cap][3]
array, and per view its pose, its feature count and its features' landmarks.  Where the project departs from the reference
(the first observation's colour, the rows that are skipped and counted, a mean over nothing) the departure is
stated here in the same plain terms."""
import numpy as np

OK, OVERFLOW, BAD_TABLE = range(3)
CAMERA_COLOR = (255, 0, 255)
CORNERS = ((1, 1), (1, -1), (-1, -1), (-1, 1))        # export.rs:98: (up, right) of up_right, up_left, down_left, down_right


def pose4(p12):
    m = np.eye(4)
    m[:3] = np.asarray(p12, np.float64).reshape(3, 4)
    return m


def points(world, rows, colors, n_blocks, cap):
    """lib.rs:2292-2307 -> ([(key, xyz, colour)], [skipped for None, skipped for w == 0, skipped for their list])"""
    out, skipped = [], [0, 0, 0]
    for key, (x, y, z, w) in enumerate(np.asarray(world, np.float64).reshape(-1, 4)):     # the SlotMap's order
        if w < 0:                                         # triangulate_landmark_robust: None
            skipped[0] += 1
        elif not w > 0:                                   # Projective::point(): None (a NaN is not a point here either)
            skipped[1] += 1
        else:
            row = rows[key] if key < len(rows) else []
            # the reference would panic on a landmark without observations; a first observation outside the colour table is
            # not something it can hold.  Both are skipped here, and counted
            if not row or row[0][0] >= n_blocks or row[0][1] >= cap:
                skipped[2] += 1
            else:
                block, feature = row[0]                   # `observations.iter().next()`: here the first of the list
                out.append((key, np.array([x, y, z]) / w, tuple(int(c) for c in colors[block][feature])))
    return out, skipped


def camera(pose12, count, cap, view_landmarks, world):
    """lib.rs:2315-2331 for one view -> dict(center, up, forward, focal_length)"""
    world = np.asarray(world, np.float64).reshape(-1, 4)
    pose = pose4(pose12)
    distances = []
    for feature in range(min(int(count), cap)):
        landmark = int(view_landmarks[feature])
        if landmark >= len(world) or world[landmark][3] < 0:
            continue
        p = pose @ world[landmark]
        if p[3] == 0:
            continue
        distances.append(float(np.linalg.norm(p[:3] / p[3])))
    mean = float(np.mean(distances)) if distances else 0.0               # the project's rule for a mean over nothing
    c2w = np.linalg.inv(pose)
    return dict(center=(c2w @ np.array([0.0, 0.0, 0.0, 1.0]))[:3], up=c2w[:3, :3] @ np.array([0.0, -1.0, 0.0]),
                forward=c2w[:3, :3] @ np.array([0.0, 0.0, 1.0]), focal_length=mean * 0.01, counted=len(distances))


def frustum(cam):
    """export.rs:95-106 -> the five vertices of a camera, the centre first"""
    c, up, fwd, f = cam["center"], cam["up"], cam["forward"], cam["focal_length"]
    right = np.cross(fwd, up)
    return [c] + [c + fwd * f + u * up * f + r * right * f for u, r in CORNERS]


def faces(n_cameras):
    """export.rs:108-113: four triangles per camera"""
    out = []
    for v in range(n_cameras):
        center, up_right, up_left, down_left, down_right = range(5 * v, 5 * v + 5)
        out += [(center, down_right, up_right), (center, up_right, up_left), (center, up_left, down_left), (center, down_left, down_right)]
    return out


def export(world, rows, colors, view_blocks, counts, landmarks, poses, cap, n_blocks, room):
    """-> dict(verdict, counts [points, None, w == 0, bad rows], keys, vertices [[x, y, z]], colors [(r, g, b)], cameras [dict],
    faces): the vertices in the file's order — the cameras' first, then the first `room` points"""
    pts, skipped = points(world, rows, colors, n_blocks, cap)
    cams = [camera(poses[b], counts[b], cap, landmarks[b], world) for b in view_blocks]
    vertices, vcolors = [], []
    for cam in cams:
        vertices += frustum(cam)
        vcolors += [CAMERA_COLOR] * 5
    written = pts[:room]
    vertices += [p for _, p, _ in written]
    vcolors += [c for _, _, c in written]
    return dict(verdict=OVERFLOW if len(pts) > room else OK, counts=[len(pts)] + skipped, keys=[k for k, _, _ in written],
                vertices=np.array(vertices, np.float64).reshape(-1, 3), colors=vcolors, cameras=cams, faces=faces(len(cams)))
