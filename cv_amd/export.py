"""Host-side mirror of cv-sfm's export of a reconstruction, over rs_export_reconstruction_device and rs_write_ply of
include/akz.h.

  VSlam::export_reconstruction   cv-sfm/src/lib.rs:2285-2340
  export                         cv-sfm/src/export.rs

The point cloud, its colours and the cameras' frusta are made on the device (cv_amd/csrc/rs_export.hip); there is no CPU
fallback.  Only the text of the .ply file is host code (rs_write_ply, in the library).  The colour table the export reads is
Akaze.sample_colors_device's.  reconstruction.export_reconstruction chains the export, one wait, the copy of the used rows and
the file.  The rules that are not the reference's (the first observation's colour, a mean over nothing, the product orders, the
number text) are in DESIGN.md §7.
"""
from dataclasses import dataclass

import numpy as np

from . import _device, _lib
from ._device import call, host_u32 as u32

VERDICTS = ("ok", "overflow", "bad_table")
CAMERA_COLOR = (255, 0, 255)


@dataclass
class ExportTensors:
    """What an rs_export_reconstruction_device call wrote, on the device (its outputs by their names without d_)."""
    xyz: object           # [5 * n_views + room][3] float64: the cameras' vertices, then the points
    rgb: object           # [5 * n_views + room][3] uint8
    key: object           # [room] int32: the landmark of point k
    cameras: object       # [n_views][RS_EX_CAMERA_WORDS] float64 {centre, up, forward, focal length}
    counts_out: object    # [RS_EX_COUNTS] int32 {points, skipped w < 0, skipped w == 0, bad rows}
    verdict: object       # [1] int32 (RS_EX_*)
    n_views: int
    room: int


@dataclass
class ExportResult:
    xyz: np.ndarray       # [5 * n_views + points written][3]
    rgb: np.ndarray       # [5 * n_views + points written][3] uint8
    key: np.ndarray       # [points written] uint32
    cameras: np.ndarray   # [n_views][RS_EX_CAMERA_WORDS]
    counts: np.ndarray    # [RS_EX_COUNTS] uint32
    verdict: int
    n_views: int
    tensors: object       # the ExportTensors it was read from


class ReconstructionExport:
    """The export of a reconstruction on the context (and stream) of an EssentialConsensus, so that it queues behind that
    object's other calls."""

    def __init__(self, consensus):
        self._cons = consensus

    def export_device(self, d_world, n_world, d_obs_start, d_obs, n_obs, n_landmarks, d_colors, view_blocks, d_counts, d_landmarks, cap, n_blocks,
                      d_poses, room, d_xyz, d_rgb, d_key, d_cameras, d_counts_out, d_verdict, stream_to_wait=None):
        """rs_export_reconstruction_device: d_* and stream_to_wait as _device.arg / wait take them, view_blocks a sequence of
        blocks.  Enqueues and returns."""
        blocks, n = _device.index_list(view_blocks)
        call("rs_export_reconstruction_device", self._cons._h, d_world, n_world, d_obs_start, d_obs, n_obs, n_landmarks, d_colors, blocks, n,
             d_counts, d_landmarks, cap, n_blocks, d_poses, room, d_xyz, d_rgb, d_key, d_cameras, d_counts_out, d_verdict,
             _device.wait(stream_to_wait))

    def export_tensors(self, torch, table, world, colors, view_blocks, counts, landmarks, cap, d_poses, room=None, n_world=None,
                       stream_to_wait=None):
        """The export of the reconstruction whose landmark table is `table` (a LandmarkTable) and whose views are
        `view_blocks`: world [n_world][4] float64, colors [n_blocks][cap][3] uint8, counts [n_blocks], landmarks [n_blocks][cap]
        (a landmarks_out): numpy arrays or device tensors; d_poses [n_blocks][12] float64 device tensor.  room: the points the
        outputs can hold (default: one per row of the world table, which cannot overflow).  Enqueued behind the current torch
        stream (or stream_to_wait); no wait -> ExportTensors."""
        dev = d_poses.device
        _device.require_device(d_poses, itemsize=8)
        n_blocks = int(d_poses.shape[0])
        ins = [_device.tensor(torch, world, np.float64, dev), _device.tensor(torch, colors, np.uint8, dev), _device.tensor(torch, counts, np.uint32, dev),
               _device.tensor(torch, landmarks, np.uint32, dev)]
        n_world = int(np.prod(world.shape)) // 4 if n_world is None else n_world
        room = n_world if room is None else room
        n_views = len(view_blocks)
        rows = _lib.RS_EX_CAMERA_VERTICES * n_views + room
        o = ExportTensors(torch.zeros((rows, 3), dtype=torch.float64, device=dev), torch.zeros((rows, 3), dtype=torch.uint8, device=dev),
                          torch.zeros((max(room, 1),), dtype=torch.int32, device=dev),
                          torch.zeros((n_views, _lib.RS_EX_CAMERA_WORDS), dtype=torch.float64, device=dev),
                          torch.zeros((_lib.RS_EX_COUNTS,), dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev), n_views, room)
        self.export_device(ins[0], n_world, table.d_start, table.d_obs, table.n_obs, table.n_landmarks, ins[1], view_blocks, ins[2], ins[3], cap,
                           n_blocks, d_poses, room, o.xyz, o.rgb, o.key, o.cameras, o.counts_out, o.verdict,
                           _device.wait_or_current(torch, stream_to_wait, dev))
        return _device.keep_alive(o, ins, table, d_poses)

    def run_export(self, torch, *args, **kw):
        """export_tensors, then WAITS and copies the used rows to the host -> ExportResult"""
        o = self.export_tensors(torch, *args, **kw)
        self._cons.sync()
        return to_host(o)


def to_host(o):
    """An ExportTensors whose stream has been waited for -> ExportResult: the cameras' vertices and the points written."""
    counts = u32(o.counts_out)
    n = min(int(counts[_lib.RS_EX_C_POINTS]), o.room)
    rows = _lib.RS_EX_CAMERA_VERTICES * o.n_views + n
    return ExportResult(o.xyz[:rows].cpu().numpy(), o.rgb[:rows].cpu().numpy(), u32(o.key[:n]) if n else np.zeros(0, np.uint32),
                        o.cameras.cpu().numpy(), counts, int(u32(o.verdict)[0]), o.n_views, o)


def write_ply(path, xyz, rgb, n_cameras, camera_faces=True):
    """rs_write_ply: the file export.rs writes, from host arrays xyz [n][3] float64 and rgb [n][3] uint8 whose first
    5 * n_cameras rows are the cameras' vertices."""
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    if len(xyz) != len(rgb):
        raise ValueError("one colour per vertex")
    _lib.check(_lib.lib().rs_write_ply(str(path).encode(), xyz.ctypes.data if len(xyz) else None, rgb.ctypes.data if len(rgb) else None, len(xyz),
                                       n_cameras, int(bool(camera_faces))), "rs_write_ply")


def read_ply(path):
    """An ASCII .ply as write_ply writes it -> (xyz [n][3] float64, rgb [n][3] uint8, faces [m][3] int32 or None, comments)."""
    with open(path) as fp:
        lines = fp.read().split("\n")
    if lines[:2] != ["ply", "format ascii 1.0"]:
        raise ValueError("not an ASCII .ply")
    end = lines.index("end_header")
    elements, comments = [], []
    for line in lines[2:end]:
        word = line.split()
        if word[0] == "comment":
            comments.append(line[len("comment "):])
        elif word[0] == "element":
            elements.append([word[1], int(word[2]), []])
        elif word[0] == "property":
            elements[-1][2].append(word[1:])
    sizes = {name: n for name, n, _ in elements}
    props = {name: p for name, _, p in elements}
    if [e[0] for e in elements] not in (["vertex"], ["vertex", "face"]) or props["vertex"] != [["double", "x"], ["double", "y"], ["double", "z"],
                                                                                              ["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]]:
        raise ValueError("not the vertex element export.rs declares")
    if "face" in props and props["face"] != [["list", "uchar", "int", "vertex_index"]]:
        raise ValueError("not the face element export.rs declares")
    n = sizes["vertex"]
    body = [line.split() for line in lines[end + 1:end + 1 + n]]
    xyz = np.array([[float(v) for v in row[:3]] for row in body], np.float64).reshape(n, 3)
    rgb = np.array([[int(v) for v in row[3:6]] for row in body], np.uint8).reshape(n, 3)
    faces = None
    if "face" in sizes:
        rows = [line.split() for line in lines[end + 1 + n:end + 1 + n + sizes["face"]]]
        if any(row[0] != "3" or len(row) != 4 for row in rows):
            raise ValueError("faces are triangles")
        faces = np.array([[int(v) for v in row[1:]] for row in rows], np.int32).reshape(len(rows), 3)
    return xyz, rgb, faces, comments
