"""The repacking of a reconstruction, written from the reference's text in dicts and lists — no arrays, no scans, nothing
shared with include/akz_repack_math.h or the kernels.

  VSlamData::remove_view                   cv-sfm/src/lib.rs:517-546

A reconstruction here is what the reference keeps: landmarks {key: {view: feature}} (Landmark::observations, a map from the
view to the feature), views {view: [landmark per feature]} (View::landmarks), constraints a list of ((v0, v1, v2), payload)
and frames a list of [reconstruction, view] or [None, None] (Frame::view).  remove_view follows the reference line by line
and is applied one view at a time; then the rows are renumbered in ascending key and the blocks through the map, which is
all the device adds to it.  A landmark without observations (a tombstone, where the reference panics) is left
alone by remove_view and dropped at the renumbering."""

NONE = 0xFFFFFFFF


def from_table(start, obs, n_landmarks, n_blocks, cap):
    """CSR lists -> (landmarks, views).  The table must be the reference's kind: a view at most once in a row, a feature of a
    view in at most one row."""
    landmarks = {}
    views = {v: [None] * cap for v in range(n_blocks)}
    for key in range(n_landmarks):
        row = {}
        for i in range(int(start[key]), int(start[key + 1])):
            view, feature = int(obs[i][0]), int(obs[i][1])
            assert view not in row and views[view][feature] is None, "not a table the reference could hold"
            row[view] = feature
            views[view][feature] = key
        landmarks[key] = row
    return landmarks, views


def remove_view(landmarks, views, constraints, frames, reconstruction, view):
    """lib.rs:517-546, in its order."""
    # Remove the frame assignment to this view (:519).
    for frame in frames:
        if frame[0] == reconstruction and frame[1] == view:
            frame[0], frame[1] = None, None
    # Remove the observations corresponding to this view (:521-537).
    taken, views[view] = views[view], []
    for landmark in taken:
        if landmark is None:
            continue
        n = len(landmarks[landmark])
        assert n != 0, "landmark had 0 observations"
        if n == 1:
            del landmarks[landmark]
        else:
            del landmarks[landmark][view]
    # Remove all constraints containing this view (:539-542).
    constraints[:] = [c for c in constraints if view not in c[0]]
    # Remove the view itself (:544).
    del views[view]


def renumber(landmarks, block_map, n_landmarks, recon_start=None):
    """Rows in ascending key, blocks through the map -> (rows, key_of, recon_start_out): rows a list of lists of
    (new block, feature) in the row's order, key_of {old key: new key} for the rows kept."""
    rows, key_of = [], {}
    for key in sorted(landmarks):
        if not landmarks[key]:
            continue                                     # a tombstone: the reference has no such row
        key_of[key] = len(rows)
        rows.append([(block_map[v], f) for v, f in landmarks[key].items()])
    ranges = None
    if recon_start is not None:
        ranges = [sum(1 for k in key_of if k < int(s)) for s in recon_start]
    return rows, key_of, ranges


def repack(start, obs, n_landmarks, n_blocks, cap, block_map, order, constraints=(), frames=(), reconstruction=0, recon_start=None):
    """The whole statement: the views `order` lists (every view the map removes, in any order) are removed one at a time, then
    everything is renumbered.  block_map: a list, NONE for a removed view.  -> dict of what is left."""
    assert sorted(order) == [v for v in range(n_blocks) if block_map[v] == NONE]
    landmarks, views = from_table(start, obs, n_landmarks, n_blocks, cap)
    constraints = [(tuple(int(v) for v in c[0]), c[1]) for c in constraints]
    frames = [list(f) for f in frames]
    for view in order:
        remove_view(landmarks, views, constraints, frames, reconstruction, view)
    rows, key_of, ranges = renumber(landmarks, block_map, n_landmarks, recon_start)
    for frame in frames:
        if frame[0] == reconstruction and frame[1] is not None:
            frame[1] = block_map[frame[1]]
    return dict(rows=rows, key_of=key_of, recon_start=ranges, views_left=sorted(views),
                constraints=[(tuple(block_map[v] for v in c[0]), c[1]) for c in constraints], frames=frames)
