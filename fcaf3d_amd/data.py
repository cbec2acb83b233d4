"""The data side of a training run (what the reference gets from mmdet3d/datasets/builder.py + torch's DataLoader workers running
the pipelines of configs/fcaf3d/*.py): the datasets by their reference names, the whole set RESIDENT in device memory, and a
loader whose batches are built by ONE kernel launch from a descriptor table (csrc_post/batch.hip fc_batch_augment_voxelize).

  DATASETS / build_dataset     ScanNetDataset / SUNRGBDDataset / S3DISDataset (scannet_dataset.py:70-117, sunrgbd_dataset.py,
                               s3dis_dataset.py over custom_3d.py), RepeatDataset / ConcatDataset (mmdet's dataset_wrappers.py) —
                               built from the reference's `data.train` / `data.val` dicts unchanged
  ResidentScenes               every scene's raw points once, in one arena (ΣN, C) fp32 on the device, plus offsets
  DeviceLoader                 the FCAF3D train pipeline (or the single-augmentation test pipeline) drawn on the host from a
                               counter-based generator, applied in the batch kernel: no device read-back, no sort, one launch
  AugDeviceLoader              test-time augmentation: the A copies MultiScaleFlipAug3D asks for of each of B scenes, one launch

Stated differences to the reference:
  * filter_empty_gt=True DROPS scenes without boxes when the dataset is built; the reference keeps them in the list and re-draws
    another index when it meets one (custom_3d.py:271-289), so its epochs are as long as the unfiltered set.
  * Epoch order (a choice: mmdet's samplers are not part of the reference tree): a permutation from torch.Generator(seed + epoch),
    padded by wrapping to a multiple of world_size x samples_per_gpu, rank r takes [r::world_size].
  * Every draw is a pure function of (seed, epoch, dataset index) — Philox keyed on them — not of how many draws came before: a
    resumed run and a straight run see the same batches.
  * IndoorPointSample draws with a keyed Feistel permutation in the kernel (n distinct rows, uniform: tests/test_batch_cpu.py),
    not numpy's generator.
Streaming a set that does not fit the device from host memory is out of scope: ResidentScenes raises.
"""
import math
import os

import numpy as np
import torch

from . import _lib as L
from .pipelines import IndoorInfoDataset, flip_bev, rot_scale_trans
from .registry import Registry

DATASETS = Registry('dataset')
DESC_WORDS = 18                      # include/fcaf3d_hip.h FC_BATCH_DESC_WORDS
MAX_SCENES = 256                     # scenes per launch (csrc_post/batch.hip BATCH_MAX_SCENES)


# ---- datasets ----------------------------------------------------------------------------------------------------------------------------
class _IndoorDataset(IndoorInfoDataset):
    """The constructor keys of the reference's indoor datasets (custom_3d.py:50-93).  `pipeline` is kept as the list of dicts it
    is: DeviceLoader reads its parameters.  Indexing goes through `scene(i)` -> (dataset that owns the file, local index)."""
    WITH_YAW = False

    def __init__(self, data_root, ann_file, pipeline=None, classes=None, modality=None, box_type_3d='Depth', filter_empty_gt=True,
                 test_mode=False, **unused):
        assert box_type_3d == 'Depth', 'the indoor sets are Depth-mode'
        load = next((p for p in (pipeline or []) if p['type'] == 'LoadPointsFromFile'), {})
        use_dim = load.get('use_dim', (0, 1, 2, 3, 4, 5))
        super().__init__(data_root, ann_file, with_yaw=self.WITH_YAW, load_dim=load.get('load_dim', 6),
                         use_dim=tuple(range(use_dim)) if isinstance(use_dim, int) else tuple(use_dim))
        self.pipeline, self.CLASSES, self.test_mode = list(pipeline or []), classes, test_mode
        self.filter_empty_gt = filter_empty_gt and not test_mode
        if self.filter_empty_gt:
            self.data_infos = [i for i in self.data_infos if i.get('annos', dict(gt_num=0))['gt_num'] != 0]

    def scene(self, index):
        return self, index

    def gt_annos(self):
        """the `annos` dicts indoor_eval takes (custom_3d.py:evaluate)"""
        return [i.get('annos', dict(gt_num=0)) for i in self.data_infos]


@DATASETS.register_module()
class ScanNetDataset(_IndoorDataset):
    pass


@DATASETS.register_module()
class S3DISDataset(_IndoorDataset):
    pass


@DATASETS.register_module()
class SUNRGBDDataset(_IndoorDataset):
    WITH_YAW = True


@DATASETS.register_module()
class RepeatDataset:
    """mmdet RepeatDataset: index i is scene i % len(dataset)"""

    def __init__(self, dataset, times):
        self.dataset, self.times = build_dataset(dataset), int(times)
        self.pipeline = self.dataset.pipeline

    def __len__(self):
        return self.times * len(self.dataset)

    def scene(self, index):
        if not 0 <= index < len(self):
            raise IndexError(index)
        return self.dataset.scene(index % len(self.dataset))


@DATASETS.register_module()
class ConcatDataset:
    """mmdet ConcatDataset: the datasets back to back (S3DIS: one per area)"""

    def __init__(self, datasets, separate_eval=True):
        self.datasets = [build_dataset(d) for d in datasets]
        self.cum = np.cumsum([len(d) for d in self.datasets])
        self.pipeline = self.datasets[0].pipeline

    def __len__(self):
        return int(self.cum[-1]) if len(self.cum) else 0

    def scene(self, index):
        if not 0 <= index < len(self):
            raise IndexError(index)
        k = int(np.searchsorted(self.cum, index, side='right'))
        return self.datasets[k].scene(index - (int(self.cum[k - 1]) if k else 0))


def build_dataset(cfg):
    """mmdet3d.datasets.build_dataset: a `data.train` / `data.val` dict (or an already built dataset) -> dataset.  S3DIS configs
    pass a list of ann_files for one dataset: one dataset per file, concatenated (builder.py:24-30)."""
    if not isinstance(cfg, dict):
        return cfg
    if isinstance(cfg.get('ann_file'), (list, tuple)):
        return ConcatDataset([dict(cfg, ann_file=a) for a in cfg['ann_file']])
    if isinstance(cfg.get('ann_files'), (list, tuple)):
        cfg = dict(cfg)
        return ConcatDataset([dict(cfg, ann_file=a) for a in cfg.pop('ann_files')])
    return DATASETS.build(cfg)


# ---- the set in device memory ---------------------------------------------------------------------------------------------------------
class ResidentScenes:
    """Every scene of `dataset` loaded ONCE into one device arena (ΣN, C) fp32 of RAW points (a scene that several indices of a
    RepeatDataset / ConcatDataset name is stored once); the axis-alignment matrix stays per scene and is applied in the kernel.
    slot[i] = the arena entry of dataset index i; start / count = its rows."""

    def __init__(self, dataset, device, max_gb=64.0):
        self.dataset, self.device = dataset, torch.device(device)
        slots, files, self.slot = {}, [], np.zeros(len(dataset), np.int64)
        for i in range(len(dataset)):
            base, j = dataset.scene(i)
            key = (id(base), j)
            if key not in slots:
                slots[key] = len(files)
                files.append((base, j))
            self.slot[i] = slots[key]
        dims = {len(b.use_dim) for b, _ in files}
        assert len(dims) <= 1, 'every scene must keep the same columns'
        self.C = dims.pop() if dims else 6
        paths = [os.path.join(b.data_root, b.data_infos[j]['pts_path']) for b, j in files]
        rows = [os.path.getsize(p) // (4 * b.load_dim) for p, (b, _) in zip(paths, files)]
        need = sum(rows) * self.C * 4
        if need > max_gb * 2 ** 30:
            raise MemoryError(f'the dataset ({len(files)} scenes, {need / 2 ** 30:.2f} GB of points) does not fit the resident arena of '
                              f'max_gb={max_gb}: raise max_gb or train on a subset (streaming from host memory is not implemented)')
        self.count = np.asarray(rows, np.int64)
        self.start = np.concatenate([[0], np.cumsum(self.count)])[:-1].astype(np.int64) if rows else np.zeros(0, np.int64)
        self.arena = torch.empty((int(sum(rows)), self.C), dtype=torch.float32, device=self.device)
        self.align, self.boxes, self.labels, self.metas = [], [], [], []
        for k, ((b, j), p) in enumerate(zip(files, paths)):
            pts = np.fromfile(p, dtype=np.float32).reshape(-1, b.load_dim)[:, list(b.use_dim)]
            assert len(pts) == rows[k] and len(pts) >= 1, p
            self.arena[int(self.start[k]):int(self.start[k]) + rows[k]].copy_(torch.from_numpy(np.ascontiguousarray(pts)))
            ann = b.get_ann_info(j)
            self.align.append(ann.get('axis_align_matrix'))
            self.boxes.append(ann['gt_bboxes_3d'].tensor.clone())                     # CPU (m,7) bottom centre
            self.labels.append(ann['gt_labels_3d'].clone())
            self.metas.append(dict(sample_idx=b.data_infos[j]['point_cloud']['lidar_idx'], pts_filename=p, with_yaw=b.with_yaw))
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)        # every stream that will read the arena starts after its last write

    def __len__(self):
        return len(self.slot)


# ---- the pipeline as parameters --------------------------------------------------------------------------------------------------------
_TRAIN_STEPS = ('LoadPointsFromFile', 'LoadAnnotations3D', 'GlobalAlignment', 'IndoorPointSample', 'RandomFlip3D',
                'GlobalRotScaleTrans', 'DefaultFormatBundle3D', 'Collect3D')


def parse_pipeline(pipeline_cfg):
    """The FCAF3D train pipeline, or the single-augmentation test pipeline (MultiScaleFlipAug3D with one scale and flip=False
    around GlobalRotScaleTrans / RandomFlip3D / IndoorPointSample), as the parameters the batch kernel needs.  Any other step is
    an error that names it: there is no per-scene fallback."""
    P = dict(num_points=None, flip_h=0.0, flip_v=0.0, rot_range=(0.0, 0.0), scale_range=(1.0, 1.0), trans_std=(0.0, 0.0, 0.0),
             align=False, train=True, fixed_scale=None)
    steps = []
    for st in pipeline_cfg:
        if st['type'] == 'MultiScaleFlipAug3D':
            ratios = st.get('pts_scale_ratio', 1.0)
            ratios = ratios if isinstance(ratios, (list, tuple)) else [ratios]
            if st.get('flip', False) or len(ratios) != 1 or isinstance(st.get('img_scale'), list) and len(st['img_scale']) != 1:
                raise NotImplementedError('DeviceLoader: MultiScaleFlipAug3D with more than one augmentation is not a loader pipeline '
                                          '(test-time augmentation goes through pipelines.MultiScaleFlipAug3D and aug_test)')
            P['train'], P['fixed_scale'] = False, float(ratios[0])
            steps.extend(st['transforms'])
        else:
            steps.append(st)
    for st in steps:
        t = st['type']
        if t not in _TRAIN_STEPS:
            raise NotImplementedError(f'DeviceLoader: pipeline step {t!r} is not part of the FCAF3D pipelines the batch kernel '
                                      f'implements ({", ".join(_TRAIN_STEPS)})')
        if t == 'GlobalAlignment':
            assert st.get('rotation_axis', 2) == 2
            P['align'] = True
        elif t == 'IndoorPointSample':
            P['num_points'] = int(st['num_points'])
        elif t == 'RandomFlip3D':
            if st.get('sync_2d', True):
                raise NotImplementedError("DeviceLoader: pipeline step 'RandomFlip3D' with sync_2d=True (image flips) is not implemented")
            P['flip_h'], P['flip_v'] = float(st.get('flip_ratio_bev_horizontal', 0.0)), float(st.get('flip_ratio_bev_vertical', 0.0))
        elif t == 'GlobalRotScaleTrans':
            r = st.get('rot_range', (-0.78539816, 0.78539816))
            P['rot_range'] = (-r, r) if isinstance(r, (int, float)) else tuple(r)
            P['scale_range'] = tuple(st.get('scale_ratio_range', (0.95, 1.05)))
            s = st.get('translation_std', (0, 0, 0))
            P['trans_std'] = (s,) * 3 if isinstance(s, (int, float)) else tuple(s)
            assert not st.get('shift_height', False)
    if not P['train']:
        P['flip_h'] = P['flip_v'] = 0.0                # MultiScaleFlipAug3D(flip=False) presets both flags to False
    return P


def parse_aug_pipeline(pipeline_cfg):
    """A test pipeline whose MultiScaleFlipAug3D may ask for several augmentations (test-time augmentation: flip=True with BEV flips,
    several pts_scale_ratio) -> (P, augs): the parameters `parse_pipeline` returns for the pipeline with ONE augmentation, and the list
    of (pts_scale_ratio, pcd_horizontal_flip, pcd_vertical_flip) in the loop order of pipelines.MultiScaleFlipAug3D (img_scale ->
    pts_scale_ratio -> horizontal -> vertical).  A pipeline without MultiScaleFlipAug3D: one identity augmentation.  More than one
    img_scale, or with flip=True more than one flip_direction (they would repeat every copy), flips or scales asked for without the inner step that applies
    them, or an inner step the batch kernel does not implement: an error that names it."""
    augs, single = [(1.0, False, False)], []
    for st in pipeline_cfg:
        if st['type'] != 'MultiScaleFlipAug3D':
            single.append(st)
            continue
        for key in ('img_scale', 'flip_direction'):
            if isinstance(st.get(key), list) and len(st[key]) != 1 and (key == 'img_scale' or st.get('flip', False)):
                raise NotImplementedError(f'AugDeviceLoader: MultiScaleFlipAug3D with {len(st[key])} entries in {key!r} is not '
                                          'implemented (every augmentation would be repeated once per entry)')
        ratios = st.get('pts_scale_ratio', 1.0)
        ratios = [float(r) for r in (ratios if isinstance(ratios, (list, tuple)) else [ratios])]
        flip = bool(st.get('flip', False))
        h_aug = [False, True] if flip and st.get('pcd_horizontal_flip', False) else [False]
        v_aug = [False, True] if flip and st.get('pcd_vertical_flip', False) else [False]
        augs = [(r, h, v) for r in ratios for h in h_aug for v in v_aug]
        inner = {t['type'] for t in st['transforms']}
        if any(h or v for _, h, v in augs) and 'RandomFlip3D' not in inner:
            raise NotImplementedError("AugDeviceLoader: MultiScaleFlipAug3D asks for flips but its transforms hold no 'RandomFlip3D'")
        if any(r != 1.0 for r, _, _ in augs) and 'GlobalRotScaleTrans' not in inner:
            raise NotImplementedError("AugDeviceLoader: MultiScaleFlipAug3D asks for pts_scale_ratio but its transforms hold no "
                                      "'GlobalRotScaleTrans'")
        single.append(dict(st, flip=False, pts_scale_ratio=ratios[0]))
    return parse_pipeline(single), augs


def draw(P, seed, epoch, index):
    """The draws of one scene — flips, angle, scale, translation, sample seed — as a pure function of (seed, epoch, dataset
    index): Philox keyed on them, a counter-based generator (no state carried from one scene to the next)."""
    g = np.random.Generator(np.random.Philox(key=[int(seed) & (2 ** 64 - 1), (int(epoch) << 40) ^ int(index)]))
    u = g.random(4)
    n = g.standard_normal(3)
    return dict(flip_h=bool(u[0] < P['flip_h']), flip_v=bool(u[1] < P['flip_v']),
                angle=float(P['rot_range'][0] + u[2] * (P['rot_range'][1] - P['rot_range'][0])),
                scale=float(P['scale_range'][0] + u[3] * (P['scale_range'][1] - P['scale_range'][0])) if P['fixed_scale'] is None
                else P['fixed_scale'],
                trans=[float(n[i] * P['trans_std'][i]) for i in range(3)],
                sample_seed=int(g.integers(0, 2 ** 64, dtype=np.uint64)))


def epoch_order(n, seed, epoch, samples_per_gpu, world_size=1, shuffle=True, pad=None):
    """dataset indices of an epoch for ALL ranks: a permutation from torch.Generator(seed + epoch) (shuffle=False: 0 .. n-1),
    padded by wrapping to a multiple of world_size x samples_per_gpu so that every rank takes the same number of full steps
    (pad, default = shuffle; a validation set is not padded: a scene scored twice would change the result); rank r takes
    [r::world_size]"""
    if shuffle:
        g = torch.Generator()
        g.manual_seed(int(seed) + int(epoch))
        order = torch.randperm(n, generator=g).numpy().astype(np.int64)
    else:
        order = np.arange(n, dtype=np.int64)
    if (shuffle if pad is None else pad) and n:
        unit = world_size * samples_per_gpu
        order = np.resize(order, (n + unit - 1) // unit * unit)
    return order


# ---- a batch -------------------------------------------------------------------------------------------------------------------------------
class _ScenePoints:
    """One scene of a DeviceBatch, with the surface of a points tensor that the detector's consumers use: .shape, .device,
    voxelize_into (the per-scene route of SingleStageSparse3DDetector.voxelize, through the same kernel)."""

    def __init__(self, batch, b, n_out, C):
        self.batch, self.b = batch, b
        self.shape, self.device = (n_out, C), batch.resident.device
        self.is_cuda = self.device.type == 'cuda'         # SingleStageSparse3DDetector.prefetch plans ahead for device-resident points only

    def voxelize_into(self, batch_idx, voxel_size, feat_div, coords, feats, points_out=None):
        n = self.shape[0]
        d = self.batch.desc[self.b:self.b + 1].copy()
        d[0, 3] = 0
        self.batch._launch(d, n, voxel_size, feat_div, coords, feats, points_out)
        if batch_idx:
            coords[:n, 0] = batch_idx

    def materialize(self):
        n, C = self.shape
        out = torch.empty((n, C), dtype=torch.float32, device=self.device)
        coords = torch.empty((n, 4), dtype=torch.int32, device=self.device)
        feats = torch.empty((n, C - 3), dtype=torch.float32, device=self.device)
        self.voxelize_into(0, 1.0, 1.0, coords, feats, out)
        return out


class DeviceBatch(list):
    """`points` of a batch: a list of _ScenePoints that also carries the batch-level hook `voxelize_batch`, which
    SingleStageSparse3DDetector.voxelize takes when it is present — all scenes in one launch."""

    def __init__(self, resident, desc):
        self.resident, self.desc = resident, desc
        C = resident.C
        super().__init__(_ScenePoints(self, b, int(desc[b, 2]), C) for b in range(len(desc)))

    def _launch(self, desc, total, voxel_size, feat_div, coords, feats, points_out=None, sample_out=None):
        r = self.resident
        assert coords.shape[0] >= total and feats.shape[0] >= total
        dev_desc = L.upload(desc, r.device)
        L.call('fc_batch_augment_voxelize', L.ptr(r.arena), r.arena.shape[0], r.C, L.ptr(dev_desc), len(desc), int(total), int(total),
               None, 0, float(voxel_size), float(feat_div), r.C - 3, L.ptr(coords), L.ptr(feats), L.ptr(sample_out), L.ptr(points_out),
               L.stream())

    def voxelize_batch(self, voxel_size, feat_div, coords, feats, points_out=None, sample_out=None):
        self._launch(self.desc, int(self.desc[:, 2].sum()), voxel_size, feat_div, coords, feats, points_out, sample_out)


def xform_words(align, p):
    """the 24 floats of fc_augment_voxelize (pipelines.LazyAugmentedPoints.xform), as 12 int64 descriptor words"""
    x = np.zeros(24, np.float32)
    if align is not None:
        m = np.asarray(align, np.float32)
        x[0:9], x[9:12], x[12] = m[:3, :3].reshape(-1), m[:3, 3], 1.0
    x[13], x[14] = float(p['flip_h']), float(p['flip_v'])
    x[15], x[16] = math.cos(p['angle']), math.sin(p['angle'])
    x[17] = p['scale']
    x[18:21] = np.asarray(p['trans'], np.float32)
    return x.view(np.int64)


class DeviceLoader:
    """Batches of a ResidentScenes set for one rank: the dict TrainStep takes (points, gt_bboxes_3d, gt_labels_3d, img_metas).
    Nothing here touches the device: a batch is a descriptor table on the host (uploaded by the launch that reads it) and the
    ground truth as CPU tensors, moved by flip_bev / rot_scale_trans — the target assignment packs them and uploads them with one
    copy per batch.  The rotation is drawn but not applied to a scene without boxes (the reference's _rot_bbox_points).
    The batches of an epoch are built once and kept, so the object `prefetch` saw is the object the next step gets."""

    def __init__(self, resident, pipeline_cfg, samples_per_gpu, seed=0, rank=0, world_size=1, shuffle=None):
        from .boxes import DepthInstance3DBoxes
        self.resident, self.P = resident, parse_pipeline(pipeline_cfg)
        self.samples_per_gpu, self.seed, self.rank, self.world_size = int(samples_per_gpu), int(seed), int(rank), int(world_size)
        assert 1 <= self.samples_per_gpu <= MAX_SCENES, f'samples_per_gpu must be 1 .. {MAX_SCENES}'
        self.shuffle = self.P['train'] if shuffle is None else shuffle
        self.epoch = 0
        self._box_type = DepthInstance3DBoxes
        if any(a is None for a in resident.align) and self.P['align'] and len(resident.align):
            raise AssertionError('axis_align_matrix is not provided in GlobalAlignment')

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def indices(self, epoch=None):
        """this rank's dataset indices of an epoch, in order"""
        e = self.epoch if epoch is None else epoch
        return epoch_order(len(self.resident), self.seed, e, self.samples_per_gpu, self.world_size, self.shuffle,
                           pad=self.P['train'])[self.rank::self.world_size]

    def __len__(self):
        return (len(self.indices()) + self.samples_per_gpu - 1) // self.samples_per_gpu

    def draw(self, epoch, index):
        return draw(self.P, self.seed, epoch if self.P['train'] else 0, index)

    def batch(self, epoch, idx):
        r, P = self.resident, self.P
        desc = np.zeros((len(idx), DESC_WORDS), np.int64)
        boxes, labels, metas, off = [], [], [], 0
        for b, i in enumerate(idx):
            k = int(r.slot[i])
            p = self.draw(epoch, int(i))
            n_src = int(r.count[k])
            n_out = P['num_points'] if P['num_points'] is not None else n_src
            bx, with_yaw = r.boxes[k], r.metas[k]['with_yaw']
            if len(bx) == 0 and P['train']:
                p = dict(p, angle=0.0)                 # GlobalRotScaleTrans._rot_bbox_points: no boxes, no rotation
            desc[b, :6] = r.start[k], n_src, n_out, off, 0, 0
            desc[b, 4:5].view(np.uint64)[0] = p['sample_seed']
            desc[b, 6:] = xform_words(r.align[k] if P['align'] else None, p)
            off += n_out
            empty = bx.new_zeros((0, 3))
            if p['flip_h']:
                _, bx = flip_bev(empty, bx, 'horizontal', with_yaw)
            if p['flip_v']:
                _, bx = flip_bev(empty, bx, 'vertical', with_yaw)
            _, bx = rot_scale_trans(empty, bx, p['angle'], p['scale'], p['trans'], with_yaw)
            gt = self._box_type.__new__(self._box_type)
            gt.tensor, gt.box_dim, gt.with_yaw = bx, 7, with_yaw
            boxes.append(gt)
            labels.append(r.labels[k])
            metas.append(dict(box_type_3d=self._box_type, sample_idx=r.metas[k]['sample_idx'], pts_filename=r.metas[k]['pts_filename'],
                              dataset_index=int(i), pcd_horizontal_flip=p['flip_h'], pcd_vertical_flip=p['flip_v'],
                              pcd_rotation_angle=p['angle'], pcd_scale_factor=p['scale'], pcd_trans=np.asarray(p['trans'], np.float32)))
        out = dict(points=DeviceBatch(r, desc), img_metas=metas)
        if P['train']:
            out.update(gt_bboxes_3d=boxes, gt_labels_3d=labels)
        return out

    def batches(self, epoch=None):
        e = self.epoch if epoch is None else int(epoch)
        idx = self.indices(e)
        s = self.samples_per_gpu
        return [self.batch(e, idx[o:o + s]) for o in range(0, len(idx), s)]

    def __iter__(self):
        return iter(self.batches())


# ---- test-time augmentation batches ------------------------------------------------------------------------------------------------------
class AugBatch(list):
    """`points` of a test-time augmentation batch: points[a][b] = augmentation a of scene b, as aug_test takes it, and `.flat`, ONE
    DeviceBatch over the A * B copies (copy a of scene b at descriptor a * B + b) that voxelises them all in one launch"""

    def __init__(self, flat, A, B):
        self.flat = flat
        super().__init__([flat[a * B + b] for b in range(B)] for a in range(A))


class AugDeviceLoader(DeviceLoader):
    """Test-time augmentation batches of a ResidentScenes set, with DeviceLoader's surface in test mode: a batch is
    dict(points=AugBatch, img_metas=img_metas[a][b]).  The A augmentations are those of the pipeline's MultiScaleFlipAug3D
    (parse_aug_pipeline), applied to B scenes by ONE launch over A * B <= 256 descriptors.  Every copy samples its own points, as
    the reference's per-copy IndoorPointSample does: copy a of dataset index i draws with Philox keyed on (seed, (a << 40) ^ i) — a
    pure function of (seed, index, a), and for a = 0 the draw of DeviceLoader for (seed, i): when augmentation 0 is the identity,
    copy 0 is the scene DeviceLoader gives."""

    def __init__(self, resident, pipeline_cfg, samples_per_gpu, seed=0, rank=0, world_size=1):
        from .boxes import DepthInstance3DBoxes
        self.resident = resident
        self.P, self.augs = parse_aug_pipeline(pipeline_cfg)
        if self.P['train']:
            raise NotImplementedError('AugDeviceLoader: a pipeline without MultiScaleFlipAug3D is a training pipeline (DeviceLoader)')
        self.samples_per_gpu, self.seed, self.rank, self.world_size = int(samples_per_gpu), int(seed), int(rank), int(world_size)
        A = len(self.augs)
        if self.samples_per_gpu < 1 or A * self.samples_per_gpu > MAX_SCENES:
            raise ValueError(f'{A} augmentations x samples_per_gpu={self.samples_per_gpu} = {A * self.samples_per_gpu} copies in one '
                             f'launch: at most {MAX_SCENES}')
        self.shuffle, self.epoch = False, 0
        self._box_type = DepthInstance3DBoxes
        if any(a is None for a in resident.align) and self.P['align'] and len(resident.align):
            raise AssertionError('axis_align_matrix is not provided in GlobalAlignment')

    def draw(self, epoch, index, a=0):
        """the draws of copy a of dataset index `index` (the same in every epoch): augmentation a's scale and flips, its own sample seed"""
        s, h, v = self.augs[a]
        return dict(draw(self.P, self.seed, a, index), scale=s, flip_h=h, flip_v=v)

    def batch(self, epoch, idx):
        r, P = self.resident, self.P
        A, B = len(self.augs), len(idx)
        desc = np.zeros((A * B, DESC_WORDS), np.int64)
        metas, off = [], 0
        for a in range(A):
            metas.append([])
            for b, i in enumerate(idx):
                k = int(r.slot[i])
                p = self.draw(epoch, int(i), a)
                n_src = int(r.count[k])
                n_out = P['num_points'] if P['num_points'] is not None else n_src
                d = a * B + b
                desc[d, :6] = r.start[k], n_src, n_out, off, 0, 0
                desc[d, 4:5].view(np.uint64)[0] = p['sample_seed']
                desc[d, 6:] = xform_words(r.align[k] if P['align'] else None, p)
                off += n_out
                metas[a].append(dict(box_type_3d=self._box_type, sample_idx=r.metas[k]['sample_idx'],
                                     pts_filename=r.metas[k]['pts_filename'], dataset_index=int(i), pcd_horizontal_flip=p['flip_h'],
                                     pcd_vertical_flip=p['flip_v'], pcd_scale_factor=p['scale']))
        return dict(points=AugBatch(DeviceBatch(r, desc), A, B), img_metas=metas)
