"""Drop-in for the reference's ``pytorch_version/dataset.py`` (``pose_framework_KITTI``): consecutive-frame pairs of
KITTI odometry sequences with the ground-truth RELATIVE pose of the pair, used by ``validate()`` (train.py:220-247).

Same class name, constructor arguments and sample layout as the reference (dataset.py:11-77): a 6-channel float tensor
(channels 0-2 = the LATER frame, 3-5 = the earlier one, both resized to (img_height, img_width)) and the 4x4 transform
inv(T_{i}) @ T_{i+1} built from ``poses/<seq>.txt``.  The reference reads files with the removed scipy.misc functions
and the ``path`` package; this build uses PIL with the same byte-scale + bilinear semantics as ``un_dataset.py``
(parity unpinned: no reference fixture exists for image decoding)."""
import glob
import os
import random

import numpy as np
import torch
import torch.utils.data as data

from un_dataset import imread, imresize


def read_scene_data(data_root, sequence_set, step=1):
    """(image file lists, [n,3,4] pose arrays) of the sequences whose directory name matches an entry of
    ``sequence_set`` under ``<root>/sequences`` (reference dataset.py:80-97)."""
    im_sequences, poses_sequences = [], []
    seq_dirs = set()
    for seq in sequence_set:
        seq_dirs |= set(d for d in glob.glob(os.path.join(data_root, "sequences", seq)) if os.path.isdir(d))
    for d in sorted(seq_dirs):
        name = os.path.basename(d)
        poses = np.genfromtxt(os.path.join(data_root, "poses", f"{name}.txt")).astype(np.float32).reshape(-1, 3, 4)
        imgs = sorted(glob.glob(os.path.join(d, "image_2", "*.png")))
        im_sequences.append(imgs)
        poses_sequences.append(poses)
    return im_sequences, poses_sequences


class pose_framework_KITTI(data.Dataset):
    def __init__(self, root, sequence_set, step=1, transform=None, seed=2018, img_height=160, img_width=608, shuffle=True):
        np.random.seed(seed)
        random.seed(seed)
        self.shuffle = shuffle
        self.root, self.transform = root, transform
        self.img_files, self.poses = read_scene_data(self.root, sequence_set, step)
        self.sequence_num = len(self.poses)
        self.height, self.width = img_height, img_width
        self.generator()

    def generator(self):
        samples = []
        self.gt_se3 = []
        for pose_list in self.poses:                                  # relative poses inv(T_{i-1}) @ T_i  (:22-33)
            prev, rel = np.eye(4), []
            for idx in range(pose_list.shape[0]):
                cur = np.eye(4)
                cur[:3] = pose_list[idx]
                rel.append(np.linalg.inv(prev).dot(cur))
                prev = cur
            self.gt_se3.append(rel)
        for img_list, pose_list in zip(self.img_files, self.gt_se3):
            for i in range(len(img_list) - 1):
                samples.append({"imgs": [img_list[i], img_list[i + 1]], "pose": pose_list[i + 1]})
        if self.shuffle:
            random.shuffle(samples)
        self.samples = samples

    def __getitem__(self, index):
        sample = self.samples[index]
        imgs = [imread(p).astype(np.float32) for p in sample["imgs"]]
        imgs = [imresize(im, (self.height, self.width)).astype(np.float32) for im in imgs]
        if self.transform is not None:
            imgs = [t.numpy() for t in self.transform(imgs)]
        else:
            imgs = [np.transpose(im, (2, 0, 1)) for im in imgs]
        img_data = np.zeros((6, self.height, self.width), dtype=np.float32)
        img_data[:3] = imgs[1]                                        # later frame first (:60-61, :74-75)
        img_data[3:] = imgs[0]
        return torch.from_numpy(img_data).type(torch.FloatTensor), torch.from_numpy(sample["pose"]).type(torch.FloatTensor)

    def __len__(self):
        return len(self.samples)


def odometry_sequences(root, sequence_set, img_height, img_width):
    """The sequences of ``sequence_set`` under ``root`` one by one, for ``dvf.validation.validate_odometry``: a list of (name,
    pairs, poses) in directory order.  ``pairs`` is ``pose_framework_KITTI(root, [name], shuffle=False)``: its sample i is
    the frame pair (i, i + 1) in ``validate()``'s layout, in frame order; ``poses`` is the ground truth of ``poses/<name>.txt``
    as [n,3,4] float64 (``read_scene_data`` keeps float32, enough for a relative pose but not for a trajectory of kilometres),
    one pose per frame."""
    names = set()
    for seq in sequence_set:
        names |= set(os.path.basename(d) for d in glob.glob(os.path.join(root, "sequences", seq)) if os.path.isdir(d))
    out = []
    for name in sorted(names):
        pairs = pose_framework_KITTI(root, [name], img_height=img_height, img_width=img_width, shuffle=False)
        poses = np.genfromtxt(os.path.join(root, "poses", f"{name}.txt"), dtype=np.float64).reshape(-1, 3, 4)
        if len(pairs) != poses.shape[0] - 1:
            raise ValueError(f"sequence {name}: {len(pairs) + 1} frames but {poses.shape[0]} ground-truth poses")
        out.append((name, pairs, poses))
    return out


class DepthValidationSet(data.Dataset):
    """Frames with ground-truth depth for ``dvf.validation.validate_depth``.  Layout: ``root/val.txt`` holds one stem per line,
    ``root/image/<stem>.png|jpg`` the frame and ``root/depth/<stem>.npy`` a float32 [Hg,Wg] map in metres with 0 for no
    measurement (a projected LiDAR sweep).  A sample is (frame [3,img_height,img_width] float32, depth [Hg,Wg] float32): the
    frame goes through the same ``imread`` / ``imresize`` and keeps the value range (0..255) that ``un_dataset.dataset``
    hands to ``un_dataset.to_batch``; the depth keeps its own size -- the prediction is brought to it, not the other way.
    ``shapes`` lists every sample's (Hg, Wg), read once from the .npy headers (``mmap_mode='r'``: no map is loaded)."""

    def __init__(self, root, img_height, img_width):
        self.root, self.height, self.width = root, img_height, img_width
        with open(os.path.join(root, "val.txt")) as f:
            self.stems = [line.strip() for line in f if line.strip()]
        self.images = []
        for stem in self.stems:
            found = [p for p in (os.path.join(root, "image", stem + ext) for ext in (".png", ".jpg")) if os.path.exists(p)]
            if not found:
                raise FileNotFoundError(f"no image/{stem}.png or .jpg under {root}")
            self.images.append(found[0])
        self.depths = [os.path.join(root, "depth", stem + ".npy") for stem in self.stems]
        self.shapes = []
        for p in self.depths:
            shape = tuple(np.load(p, mmap_mode="r", allow_pickle=False).shape)
            if len(shape) != 2:
                raise ValueError(f"{p}: expected a [H,W] depth map, got shape {shape}")
            self.shapes.append(shape)

    def __getitem__(self, index):
        img = imresize(imread(self.images[index]).astype(np.float32), (self.height, self.width)).astype(np.float32)
        depth = np.load(self.depths[index], allow_pickle=False).astype(np.float32)
        return (torch.from_numpy(np.ascontiguousarray(np.transpose(img, (2, 0, 1)))),
                torch.from_numpy(np.ascontiguousarray(depth)))

    def __len__(self):
        return len(self.stems)

    def batches(self, batch_size):
        """Index lists for a DataLoader's ``batch_sampler``: consecutive samples of equal ground-truth size, at most
        ``batch_size`` of them, so that a batch's depth maps stack into one [B,Hg,Wg] tensor."""
        out = []
        for i, shape in enumerate(self.shapes):
            if out and len(out[-1]) < batch_size and self.shapes[out[-1][-1]] == shape:
                out[-1].append(i)
            else:
                out.append([i])
        return out

    def loader(self, batch_size, num_workers=0):
        return data.DataLoader(self, batch_sampler=self.batches(batch_size), num_workers=num_workers)


def depth_validation_set(root, img_height, img_width):
    """The depth validation set under ``root`` (see ``DepthValidationSet``); ``.loader(batch_size)`` batches it by
    ground-truth size."""
    return DepthValidationSet(root, img_height, img_width)


class KittiRawDepthSet(data.Dataset):
    """Frames of a KITTI raw tree with their LiDAR sweep and calibration, for ``dvf.validation.validate_depth`` and
    ``export_depth_tree``: the ground truth is built from the sweep on the device (``dvf.velodyne.depth_maps``), nothing is
    projected here.  A line of ``split_file`` is ``<date>/<drive>/image_0<cam>/data/<id>.png ...`` (an Eigen split list): the
    first field names the frame and later fields are ignored, as in the reference's read_file_data
    (tools/eval_depth_utils.py:79-109); the camera directory of the line is replaced by ``cam``'s.  The sweep is
    ``<date>/<drive>/velodyne_points/data/<id>.bin`` (raw float32 quadruples) and the calibration comes from
    ``dvf.velodyne.find_calib_dir``.  A listed frame whose image is absent is reported (``<path> missing``) and skipped, as the
    reference does; an absent sweep or calibration file of a present image raises with the path.

    A sample is (frame [3,img_height,img_width] float32 through the same ``imread`` / ``imresize`` as ``DepthValidationSet``,
    points [N,4] float32, proj [3,4] float64).  ``shapes`` lists every sample's ground-truth size (Hg, Wg) = the size of the
    ORIGINAL image, read from the file header without decoding; ``stems`` its ``<drive>_<id>``."""

    def __init__(self, root, split_file, img_height, img_width, cam=2):
        from PIL import Image
        from dvf.velodyne import CAMS, find_calib_dir, velo_to_image
        if cam not in CAMS:
            raise ValueError(f"KittiRawDepthSet: cam must be one of {CAMS}, got {cam!r}")
        self.root, self.height, self.width, self.cam = root, img_height, img_width, cam
        self.images, self.sweeps, self.projs, self.shapes, self.stems, self.missing = [], [], [], [], [], []
        calib = {}
        with open(split_file) as f:
            lines = [line.split()[0] for line in f if line.strip()]
        for name in lines:
            parts = name.split("/")
            if len(parts) != 5:
                raise ValueError(f"{split_file}: expected <date>/<drive>/image_0<cam>/data/<id>.png, got {name!r}")
            date, drive, frame_id = parts[0], parts[1], os.path.splitext(parts[4])[0]
            image = os.path.join(root, date, drive, f"image_0{cam}", "data", parts[4])
            if not os.path.isfile(image):
                print(f"{image} missing", flush=True)
                self.missing.append(image)
                continue
            sweep = os.path.join(root, date, drive, "velodyne_points", "data", frame_id + ".bin")
            if not os.path.isfile(sweep):
                raise FileNotFoundError(f"{sweep}: no LiDAR sweep for {image}")
            calib_dir = find_calib_dir(root, date, drive)
            if calib_dir not in calib:
                calib[calib_dir] = velo_to_image(calib_dir, cam)
            with Image.open(image) as im:                              # (the header only: nothing is decoded)
                wg, hg = im.size
            self.images.append(image)
            self.sweeps.append(sweep)
            self.projs.append(calib[calib_dir])
            self.shapes.append((hg, wg))
            self.stems.append(f"{drive}_{frame_id}")

    def frame(self, index):
        img = imresize(imread(self.images[index]).astype(np.float32), (self.height, self.width)).astype(np.float32)
        return torch.from_numpy(np.ascontiguousarray(np.transpose(img, (2, 0, 1))))

    def sweep(self, index):
        """(points [N,4] float32, proj [3,4] float64) of a sample."""
        points = np.fromfile(self.sweeps[index], dtype=np.float32)
        if points.size % 4:
            raise ValueError(f"{self.sweeps[index]}: {points.size} floats are no whole number of (x, y, z, reflectance) points")
        return torch.from_numpy(points.reshape(-1, 4)), torch.from_numpy(np.ascontiguousarray(self.projs[index], dtype=np.float64))

    def __getitem__(self, index):
        return (self.frame(index),) + self.sweep(index)

    def __len__(self):
        return len(self.images)

    batches = DepthValidationSet.batches

    def collate(self, indices, frames=True):
        """One batch of ``batches``: (frames [B,3,h,w], points [total,4], offsets [B+1] int32, proj [B,3,4] float64, (Hg, Wg)),
        the points of the B sweeps back to back and frame b owning points offsets[b] .. offsets[b+1]-1.  ``frames=False``
        decodes no image and puts None first."""
        sweeps = [self.sweep(i) for i in indices]
        offsets = torch.tensor(np.concatenate([[0], np.cumsum([p.shape[0] for p, _ in sweeps])]), dtype=torch.int32)
        return (torch.stack([self.frame(i) for i in indices]) if frames else None, torch.cat([p for p, _ in sweeps]), offsets,
                torch.stack([m for _, m in sweeps]), tuple(self.shapes[indices[0]]))

    def loader(self, batch_size, num_workers=0):
        """A DataLoader over the collated batches of ``batches(batch_size)``; ``.dataset.source`` is this set."""
        return data.DataLoader(_RawDepthBatches(self, self.batches(batch_size)), batch_size=None, shuffle=False,
                               num_workers=num_workers)


class _RawDepthBatches(data.Dataset):
    """Item i = the collated batch i of a KittiRawDepthSet (the ground-truth size of a batch is the set's knowledge, not
    the samples')."""

    def __init__(self, source, batches):
        self.source, self.batches = source, batches

    def __getitem__(self, index):
        return self.source.collate(self.batches[index])

    def __len__(self):
        return len(self.batches)


def kitti_raw_depth_set(root, split_file, img_height, img_width, cam=2):
    """The frames of ``split_file`` under the KITTI raw tree ``root`` (see ``KittiRawDepthSet``); ``.loader(batch_size)``
    batches them by ground-truth size and collates the sweeps."""
    return KittiRawDepthSet(root, split_file, img_height, img_width, cam)
