"""Ground-truth depth from KITTI raw LiDAR sweeps (csrc/velodyne.hip, ``dvf_velodyne_depth`` of include/dvf_hip.h): the device
form of the reference's generate_depth_map (tools/eval_depth_utils.py:172-224), and the calibration readers around it.

``depth_maps`` projects the sweeps of a batch of frames and keeps the nearest point of every pixel, in one call and without a
synchronisation.  ``read_calib_file`` / ``velo_to_image`` / ``find_calib_dir`` read KITTI's ``calib_cam_to_cam.txt`` and
``calib_velo_to_cam.txt`` on the host (numpy fp64: two small text files per recording day)."""
import os

import numpy as np
import torch

from . import lib as L

CAMS = (2, 3)
CALIB_FILES = ("calib_cam_to_cam.txt", "calib_velo_to_cam.txt")


def depth_maps(points, offsets, proj, H, W, velodyne_depth=False):
    """Depth maps [B,H,W] fp32 on the device from the LiDAR points of B frames: ``points`` [total,4] fp32 (forward, left, up,
    reflectance; all frames back to back), ``offsets`` [B+1] int32 on the device (frame b owns points offsets[b] ..
    offsets[b+1]-1), ``proj`` [B,3,4] fp64 on the device (``velo_to_image``).  Every point with forward >= 0 is projected in
    fp64, rounded half to even to a pixel (minus KITTI's 1) and the smallest depth of a pixel wins; negative minima and pixels
    that no point reaches are 0.  ``velodyne_depth`` stores the forward distance instead of the camera depth (the reference's
    vel_depth=True).  No synchronisation; the result is ordered on the current stream."""
    L.dev(points, "points")
    L.dev(offsets, "offsets", torch.int32)
    L.dev(proj, "proj", torch.float64)
    if points.dim() != 2 or points.shape[1] != 4:
        raise ValueError(f"depth_maps: points must be [total,4], got {tuple(points.shape)}")
    if proj.dim() != 3 or tuple(proj.shape[1:]) != (3, 4) or proj.shape[0] < 1:
        raise ValueError(f"depth_maps: proj must be [B,3,4] with B >= 1, got {tuple(proj.shape)}")
    B, total = proj.shape[0], points.shape[0]
    if offsets.dim() != 1 or offsets.numel() != B + 1:
        raise ValueError(f"depth_maps: offsets must hold B + 1 = {B + 1} entries, got {tuple(offsets.shape)}")
    depth = torch.empty(B, int(H), int(W), device=points.device, dtype=torch.float32)
    L.check(L.lib().dvf_velodyne_depth(points.data_ptr() if total else None, offsets.data_ptr(), proj.data_ptr(), depth.data_ptr(),
                                       B, int(H), int(W), total, L.VD_VELODYNE_DEPTH if velodyne_depth else 0, L.stream()),
            "dvf_velodyne_depth")
    return depth


def read_calib_file(path):
    """A KITTI calibration file (``key: values`` lines) as {key: float64 array}; a line whose values are not all numbers, such
    as ``calib_time: 09-Jan-2012 13:57:47``, keeps its string."""
    out = {}
    with open(path) as f:
        for line in f:
            if ":" not in line:
                continue
            key, value = line.split(":", 1)
            value = value.strip()
            try:
                out[key.strip()] = np.array([float(v) for v in value.split()], dtype=np.float64)
            except ValueError:
                out[key.strip()] = value
    return out


def find_calib_dir(root, date, drive):
    """The directory that holds the two calibration files of a drive: ``<root>/<date>`` (KITTI's own layout), else
    ``<root>/<date>/<drive>/calib`` (where the reference's read_file_data looks, tools/eval_depth_utils.py:100)."""
    tried = [os.path.join(root, date), os.path.join(root, date, drive, "calib")]
    for d in tried:
        if all(os.path.isfile(os.path.join(d, name)) for name in CALIB_FILES):
            return d
    raise FileNotFoundError("no " + " + ".join(CALIB_FILES) + " in " + " or ".join(tried))


def velo_to_image(calib_dir, cam=2):
    """The fp64 [3,4] matrix that takes a homogeneous velodyne point to image ``cam`` (2 = left colour, 3 = right colour):
    P_rect_0<cam> @ R_rect_00 (as 4x4) @ [R|T; 0 0 0 1] (tools/eval_depth_utils.py:174-183)."""
    if cam not in CAMS:
        raise ValueError(f"velo_to_image: cam must be one of {CAMS}, got {cam!r}")
    cam2cam = read_calib_file(os.path.join(calib_dir, CALIB_FILES[0]))
    velo2cam = read_calib_file(os.path.join(calib_dir, CALIB_FILES[1]))
    velo = np.eye(4)
    velo[:3, :3] = velo2cam["R"].reshape(3, 3)
    velo[:3, 3] = velo2cam["T"]
    rect = np.eye(4)
    rect[:3, :3] = cam2cam["R_rect_00"].reshape(3, 3)
    return cam2cam[f"P_rect_0{cam}"].reshape(3, 4).dot(rect).dot(velo)
