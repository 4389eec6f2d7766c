"""Pre-decoded image shards + the native (C++ thread pool -> pinned -> GPU augment) batch loader.

Reference input path: ``DataLoader(ImageFolderMy, num_workers=4, pin_memory=True)`` with PIL
decode and RandomResizedCrop / Resize+CenterCrop / ToTensor / Normalize on the host workers
(BASELINE/main.py:58-76,97-131) and ``inputs.cuda(non_blocking=True)`` (:273-274).  JPEG decode
plus augmentation on a few host cores tops out far below the ~14k img/s one MI355X trains
ResNet-50 at (SURVEY.md §7.5 risk 8), so this path splits the work MI355X-first:

1. **offline, once**: :func:`pack_image_folder` decodes every image (PIL, process pool), resizes
   its shorter side to ``short_side`` and appends the raw uint8 HWC pixels to one shard file
   (format below) -- variable image sizes, like the original JPEGs;
2. **per batch, host** (``csrc/host/loader.cpp``, loaded with ctypes): a std::thread pool memcpys
   the batch's records from the memory-mapped shard into a pinned slot, in the order the
   distributed sampler produced, and samples each image's crop box / flip with torchvision's
   RandomResizedCrop algorithm from a counter RNG keyed by (seed, epoch, index);
3. **per batch, device**: one H2D copy of the raw records, then ``dcp::crop_resize`` (bilinear
   crop+resize+flip, csrc/augment.hip) and ``dcp::to_nhwc`` / ``to_nhwc_s2d`` (normalise to bf16
   NHWC) on a side stream; the compute stream waits on an event only.  Presets that rotate, pad
   or stretch (CDR, CIFAR, PLC) take the affine route instead: the host also composes each
   image's resize-to-canvas, rotation, flip and crop offset into one inverse-affine matrix
   (``dcpl_submit_affine``) and ``dcp::warp_crop`` resamples the box through it, zero outside.

Shard file (little-endian)::

    Header (48 B)   magic "DCPSHRD1", u32 version=1, u32 channels=3, u64 count,
                    u64 index_off, u64 data_off, u64 max_bytes
    Index           count x {u64 offset (from data_off), u32 h, u32 w, i64 label}
    Data            records, h*w*3 uint8 each (HWC, RGB), then zero padding to 8 bytes

Differences from the PIL pipeline (documented, not hidden): the resample is plain bilinear on
the stored (short_side-resized) image, without PIL's antialiasing filter on downscales, and
Resize+CenterCrop is one resample of the centre box instead of two.  On the affine route:

* CDR's RandomResizedCrop(256) -> RandomRotation(15) -> flip -> CenterCrop(224) is ONE bilinear
  pass from the stored image to the 224 output, where PIL resamples bilinearly to 256 and then
  rotates with nearest-neighbour lookups; the geometry (box, angle about the canvas centre,
  flip, crop offset, zero fill outside the rotated canvas) is the same;
* PLC's Resize((256, 256), BICUBIC) becomes a bilinear stretch;
* CIFAR's RandomCrop(32, padding=4) -> flip is reproduced exactly (integer offsets, no resample).

``DCP_SHARD_AFFINE=0`` puts CDR, CIFAR and PLC back on the PIL DataLoader workers over the same
shard (for A/B runs); measurements in profiles/r11/loader_affine.txt.

``resample="pil"`` (``--shard-resample pil`` / ``DCP_SHARD_RESAMPLE=pil``; the default is
``"fast"``, everything above) removes every difference listed above.  The host then draws the
same boxes, angles and flips from the same streams but hands the device the integers of the PIL
chain itself (``dcpl_submit_exact``: per-image canvas size, window offset, the 16.16 map of
``Image.rotate``), and ``dcp::resample_crop`` / ``dcp::rotate_nearest_crop`` redo Pillow's
fixed-point arithmetic: the antialiased two-pass ``resize`` (bilinear, bicubic for PLC) with its
uint8 intermediate image, Resize(256) and CenterCrop(224) as two steps, CDR's canvas -> nearest
rotation -> flip -> centre crop as four.  CIFAR's pad-crop was exact already and keeps the affine
route.  What ``pil`` guarantees: for every preset, the uint8 batch equals, byte for byte, what
``transforms.build_transform(preset)`` computes on the same shard record with the same draws
(tests/test_resample_*.py compare with Pillow itself, no tolerance).  What it does not: the
shard's own one-time short-side resize at packing time is still there, and the draws are this
loader's, so a run is not equal to one that decodes the JPEGs and augments them with Python's RNG
every epoch.  Downscales above 8x per axis (33 bicubic taps) are refused, not approximated.
Measurements in profiles/r12/loader_exact.txt.
"""
from __future__ import annotations

import ctypes
import os
import struct
from collections import deque

import numpy as np
import torch

from .. import build_ext
from ..ops import functional as Fn
from .transforms import IMAGENET_MEAN, IMAGENET_STD

MAGIC = b"DCPSHRD1"
_HDR = struct.Struct("<8sIIQQQQ")  # 48 bytes
_IDX = np.dtype([("offset", "<u8"), ("h", "<u4"), ("w", "<u4"), ("label", "<i8")])  # 24 bytes
assert _HDR.size == 48 and _IDX.itemsize == 24


# ----------------------------------------------------------------------------- file format
def write_shard(path: str, samples) -> int:
    """Write ``samples`` (iterable of (uint8 HWC RGB array, int label)) to ``path``; returns count."""
    tmp = path + f".tmp{os.getpid()}"
    index = []
    off = 0
    max_bytes = 0
    with open(tmp, "wb") as f:
        f.write(b"\0" * _HDR.size)
        for img, label in samples:
            a = np.ascontiguousarray(img, dtype=np.uint8)
            if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] == 0 or a.shape[1] == 0:
                raise ValueError(f"shard records are HxWx3 uint8, got {a.shape}")
            f.write(a.tobytes())
            index.append((off, a.shape[0], a.shape[1], int(label)))
            off += a.nbytes
            max_bytes = max(max_bytes, a.nbytes)
        data_off = _HDR.size
        pad = (-(data_off + off)) % 8  # 8-byte aligned index (the records themselves are byte data)
        f.write(b"\0" * pad)
        index_off = data_off + off + pad
        idx = np.array(index, dtype=_IDX) if index else np.zeros(0, dtype=_IDX)
        f.write(idx.tobytes())
        f.seek(0)
        f.write(_HDR.pack(MAGIC, 1, 3, len(index), index_off, data_off, max_bytes))
    os.replace(tmp, path)
    return len(index)


def read_index(path: str):
    """(header dict, structured index array) of a shard file."""
    with open(path, "rb") as f:
        magic, ver, ch, count, index_off, data_off, max_bytes = _HDR.unpack(f.read(_HDR.size))
    if magic != MAGIC or ver != 1 or ch != 3:
        raise ValueError(f"{path}: not a DCPSHRD1 shard")
    idx = np.fromfile(path, dtype=_IDX, count=count, offset=index_off)
    return dict(count=count, index_off=index_off, data_off=data_off, max_bytes=max_bytes), idx


def _decode(args):
    path, label, short_side = args
    from PIL import Image

    with open(path, "rb") as fh:
        img = Image.open(fh).convert("RGB")
    if short_side:
        w, h = img.size
        s = short_side / min(w, h)
        img = img.resize((max(1, round(w * s)), max(1, round(h * s))), Image.BILINEAR)
    return np.asarray(img, dtype=np.uint8), label


def _file_list(dataset):
    if hasattr(dataset, "imgs") and hasattr(dataset, "labels"):  # CappedImageFolder / ImageFolder
        return list(zip(dataset.imgs, dataset.labels))
    if hasattr(dataset, "image_list"):  # ListDataset (paths relative to data_root)
        return [(os.path.join(dataset.data_root, p), l) for p, l in zip(dataset.image_list, dataset.label_list)]
    if hasattr(dataset, "samples"):
        return list(dataset.samples)
    raise TypeError(f"cannot list the image files of {type(dataset).__name__}")


def pack_image_folder(dataset, path: str, short_side: int = 256, workers: int = 4) -> int:
    """Decode every (path, label) of an image-folder dataset (:class:`CappedImageFolder`,
    :class:`ImageFolder`, :class:`ListDataset`) into one shard at ``path``, in dataset order."""
    samples = [(p, int(l), short_side) for p, l in _file_list(dataset)]
    if workers > 1:
        import multiprocessing as mp

        with mp.get_context("spawn").Pool(workers) as pool:
            return write_shard(path, pool.imap(_decode, samples, chunksize=16))
    return write_shard(path, map(_decode, samples))


class ShardDataset(torch.utils.data.Dataset):
    """Map-style view of a shard: ``(PIL image, label)`` (so the regular transform presets and
    DataLoader work on it) or the raw uint8 HWC array with ``raw=True``."""

    def __init__(self, path: str, transform=None, raw: bool = False):
        self.path, self.transform, self.raw = path, transform, raw
        self.hdr, self.index = read_index(path)
        self.targets = self.index["label"].astype(np.int64).tolist()
        self._mm = None

    def __len__(self):
        return int(self.hdr["count"])

    def image(self, i: int) -> np.ndarray:
        if self._mm is None:
            self._mm = np.memmap(self.path, dtype=np.uint8, mode="r")
        e = self.index[i]
        a = self.hdr["data_off"] + int(e["offset"])
        return np.asarray(self._mm[a:a + int(e["h"]) * int(e["w"]) * 3]).reshape(int(e["h"]), int(e["w"]), 3)

    def __getitem__(self, i):
        a = self.image(i)
        if self.raw:
            return a, self.targets[i]
        from PIL import Image

        img = Image.fromarray(a)
        return (self.transform(img) if self.transform else img), self.targets[i]


# ----------------------------------------------------------------------------- native library
class AugSpec(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int32), ("resize", ctypes.c_int32), ("crop", ctypes.c_int32),
                ("scale_lo", ctypes.c_float), ("scale_hi", ctypes.c_float),
                ("ratio_lo", ctypes.c_float), ("ratio_hi", ctypes.c_float), ("flip_p", ctypes.c_float),
                # read by dcpl_submit_affine / dcpl_submit_exact only; zero (the 8-field form) = no
                # rotation, no padding
                ("rot_deg", ctypes.c_float), ("pad", ctypes.c_int32),
                ("canvas_h", ctypes.c_int32), ("canvas_w", ctypes.c_int32),
                # read by the `pil` resampling mode only: 0 = bilinear, 1 = bicubic
                ("filter", ctypes.c_int32)]

    @property
    def affine(self) -> bool:
        """True when the spec needs the affine route (rotation, padding or a canvas)."""
        return bool(self.rot_deg > 0 or self.pad > 0 or self.canvas_h > 0 or self.canvas_w > 0
                    or self.mode in (MODE_PADCROP, MODE_STRETCH))


# PADCROP: RandomCrop(out, padding=pad) of the image itself; STRETCH: whole image -> fixed canvas
MODE_RRC, MODE_CENTER, MODE_WHOLE, MODE_PADCROP, MODE_STRETCH = 0, 1, 2, 3, 4


RESAMPLE_MODES = ("fast", "pil")


def aug_preset(name: str, train: bool, size: int = 224, resample: str = "fast"):
    """(AugSpec, output edge) of the reference transform presets (see transforms.build_transform).
    The geometry of a preset is the same in both resampling modes; ``resample="pil"`` adds the
    filter PIL uses (bicubic for PLC) for :class:`ShardLoader` ``(..., resample="pil")``."""
    if resample not in RESAMPLE_MODES:
        raise ValueError(f"shard resampling mode {resample!r}: one of {RESAMPLE_MODES}")
    aug, out = _aug_preset(name.lower(), train, size)
    if resample == "pil" and name.lower() == "plc":
        aug.filter = 1  # PLC/FolderDataset.py: Resize((256, 256), BICUBIC)
    return aug, out


def _aug_preset(name: str, train: bool, size: int):
    if name in ("baseline", "arcface"):
        # BASELINE/main.py:58-76: train RRC(256, scale 0.8-1), no flip; val Resize(256)+CenterCrop(224)
        if train:
            return AugSpec(MODE_RRC, 0, 0, 0.8, 1.0, 3 / 4, 4 / 3, 0.0), (size if size != 224 else 256)
        return AugSpec(MODE_CENTER, 256, size if size in (224, 256) else size, 0, 0, 1, 1, 0.0), 224 if size in (
            224, 256) else size
    if name in ("nested", "clothing1m", "imagenet"):
        # NESTED/train.py:46-65: RRC(224) + flip; val Resize(256)+CenterCrop(224)
        if train:
            return AugSpec(MODE_RRC, 0, 0, 0.08, 1.0, 3 / 4, 4 / 3, 0.5), size
        return AugSpec(MODE_CENTER, 256, size, 0, 0, 1, 1, 0.0), size
    if name in ("cdr", "plc", "cifar", "cifar10", "cifar100") and os.environ.get("DCP_SHARD_AFFINE", "1") == "0":
        raise ValueError(f"preset {name!r} needs rotation/padding and DCP_SHARD_AFFINE=0: PIL DataLoader path")
    canvas = size * 8 // 7  # the references' 256 canvas for a 224 output
    if name == "cdr":
        # CDR/main.py:112-130: train RRC(256) -> RandomRotation(15) -> flip -> CenterCrop(224)
        if train:
            return AugSpec(MODE_RRC, 0, 0, 0.08, 1.0, 3 / 4, 4 / 3, 0.5, 15.0, 0, canvas, canvas), size
        return AugSpec(MODE_CENTER, 256, size, 0, 0, 1, 1, 0.0), size
    if name in ("cifar", "cifar10", "cifar100"):
        # NESTED/train.py:40-45: RandomCrop(32, padding=4) + flip; val is the stored 32x32 image
        if train:
            return AugSpec(MODE_PADCROP, 0, 0, 1, 1, 1, 1, 0.5, 0.0, 4, 0, 0), 32
        return AugSpec(MODE_WHOLE, 0, 0, 1, 1, 1, 1, 0.0), 32
    if name == "plc":
        # PLC/FolderDataset.py: Resize((256, 256)) -> flip (train) -> CenterCrop(224); the stretch is
        # anisotropic, so validation keeps MODE_STRETCH (MODE_CENTER's box preserves the aspect ratio)
        return AugSpec(MODE_STRETCH, 0, 0, 1, 1, 1, 1, 0.5 if train else 0.0, 0.0, 0, canvas, canvas), size
    raise ValueError(f"unknown shard augmentation preset {name!r}")


_LIB = {"h": None}


def native_lib():
    """ctypes handle of ``_dcp_loader.so`` (built by build_ext.build / build_host)."""
    if _LIB["h"] is None:
        path = build_ext.LOADER_PATH
        if not os.path.exists(path):
            if os.environ.get("DCP_AUTOBUILD", "0") == "1":
                build_ext.build_host(verbose=False)
            else:
                raise RuntimeError(f"native loader not built: {path} (python -m ddp_classification_pytorch_amd.build_ext)")
        lib = ctypes.CDLL(path)
        vp, i64 = ctypes.c_void_p, ctypes.c_int64
        lib.dcpl_open.restype = vp
        lib.dcpl_open.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
        lib.dcpl_close.argtypes = [vp]
        lib.dcpl_count.restype = i64
        lib.dcpl_count.argtypes = [vp]
        lib.dcpl_pool_create.restype = vp
        lib.dcpl_pool_create.argtypes = [ctypes.c_int]
        lib.dcpl_pool_destroy.argtypes = [vp]
        lib.dcpl_submit.restype = i64
        lib.dcpl_submit.argtypes = [vp, vp, vp, ctypes.c_int, vp, i64, vp, vp, ctypes.POINTER(AugSpec),
                                    ctypes.c_uint64, ctypes.c_uint64]
        lib.dcpl_submit_affine.restype = i64
        lib.dcpl_submit_affine.argtypes = [vp, vp, vp, ctypes.c_int, vp, i64, vp, vp, vp, ctypes.POINTER(AugSpec),
                                           ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int]
        lib.dcpl_submit_exact.restype = i64
        lib.dcpl_submit_exact.argtypes = lib.dcpl_submit_affine.argtypes
        lib.dcpl_wait.restype = ctypes.c_int
        lib.dcpl_wait.argtypes = [vp, i64]
        _LIB["h"] = lib
    return _LIB["h"]


class NativeGather:
    """One memory-mapped shard + a host thread pool: ``submit(indices, slot)`` gathers records
    and samples augmentation boxes asynchronously, ``wait(ticket)`` joins."""

    def __init__(self, path: str, threads: int = 8):
        self.lib = native_lib()
        err = ctypes.create_string_buffer(512)
        self.shard = self.lib.dcpl_open(path.encode(), err, len(err))
        if not self.shard:
            raise RuntimeError("dcpl_open: " + err.value.decode())
        self.pool = self.lib.dcpl_pool_create(int(threads))
        self.hdr, _ = read_index(path)

    def __len__(self):
        return int(self.lib.dcpl_count(self.shard))

    def submit(self, indices: torch.Tensor, out: torch.Tensor, meta: torch.Tensor, labels: torch.Tensor,
               aug: AugSpec, seed: int, epoch: int, xf: torch.Tensor = None, out_hw=None,
               geo: torch.Tensor = None) -> int:
        """With ``xf`` (float32 [B, 8]) and ``out_hw`` the affine entry point also writes each image's
        inverse-affine matrix; without them this is the plain crop-box call, bit for bit.  With
        ``geo`` (int32 [B, 12]) and ``out_hw`` it is the exact entry point of the `pil` mode: the
        same draws, and each image's canvas, window offset and rotation integers."""
        assert indices.dtype == torch.int64 and indices.is_contiguous() and not indices.is_cuda
        B = indices.numel()
        assert meta.shape == (B, 8) and labels.shape == (B,) and out.dtype == torch.uint8
        if geo is not None:
            assert geo.shape == (B, 12) and geo.dtype == torch.int32 and geo.is_contiguous() and not geo.is_cuda
            t = self.lib.dcpl_submit_exact(self.pool, self.shard, indices.data_ptr(), B, out.data_ptr(),
                                           out.numel(), meta.data_ptr(), geo.data_ptr(), labels.data_ptr(),
                                           ctypes.byref(aug), int(seed) & (2**64 - 1), int(epoch),
                                           int(out_hw[0]), int(out_hw[1]))
        elif xf is None:
            if aug.affine:
                raise ValueError("this AugSpec rotates, pads or stretches: submit() needs xf and out_hw")
            t = self.lib.dcpl_submit(self.pool, self.shard, indices.data_ptr(), B, out.data_ptr(), out.numel(),
                                     meta.data_ptr(), labels.data_ptr(), ctypes.byref(aug), int(seed) & (2**64 - 1),
                                     int(epoch))
        else:
            assert xf.shape == (B, 8) and xf.dtype == torch.float32 and xf.is_contiguous() and not xf.is_cuda
            t = self.lib.dcpl_submit_affine(self.pool, self.shard, indices.data_ptr(), B, out.data_ptr(),
                                            out.numel(), meta.data_ptr(), xf.data_ptr(), labels.data_ptr(),
                                            ctypes.byref(aug), int(seed) & (2**64 - 1), int(epoch),
                                            int(out_hw[0]), int(out_hw[1]))
        if t < 0:
            raise ValueError(f"dcpl_submit rejected the batch (code {t})")
        return t

    def wait(self, ticket: int):
        rc = self.lib.dcpl_wait(self.pool, ticket)
        if rc != 0:
            raise RuntimeError(f"dcpl_wait: gather failed ({rc})")

    def close(self):
        if getattr(self, "pool", None):
            self.lib.dcpl_pool_destroy(self.pool)
            self.pool = None
        if getattr(self, "shard", None):
            self.lib.dcpl_close(self.shard)
            self.shard = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShardLoader:
    """Batches of (normalised NHWC activations, labels[, dataset index]) from a shard.

    ``sampler`` supplies the per-epoch index order (e.g. :class:`ShardSampler`, DistributedSampler
    semantics); ``prefetch`` batches are in flight (host gather -> pinned slot -> H2D -> augment)
    while the caller trains on the current one.  A slot is only refilled after the side stream's
    copy out of it has completed (event per slot).  Same yield signature as
    :class:`DevicePrefetcher`, so the training loop is unchanged.

    ``resample="pil"`` delivers the bytes of the PIL pipeline (module docstring) through
    ``dcpl_submit_exact`` and the exact kernels; the pad-crop preset keeps the affine route.
    ``tap``, when set, is called with (uint8 images, meta, xf or geo or None) of every batch before
    normalisation: tests and tools look at the augmented bytes there.
    """

    def __init__(self, path: str, batch_size: int, sampler=None, aug: AugSpec = None, out_size: int = 224,
                 device="cuda", threads: int = 8, prefetch: int = 3, seed: int = 0, drop_last: bool = False,
                 mean=IMAGENET_MEAN, std=IMAGENET_STD, cpad: int = 8, s2d=False, return_index: bool = False,
                 resample: str = "fast", mix=None):
        self.mix = mix  # a data.mix.MixSampler (train loaders only)
        if resample not in RESAMPLE_MODES:
            raise ValueError(f"shard resampling mode {resample!r}: one of {RESAMPLE_MODES}")
        self.gather = NativeGather(path, threads)
        self.batch_size, self.sampler, self.out_size = int(batch_size), sampler, int(out_size)
        self.aug = aug if aug is not None else AugSpec(MODE_WHOLE, 0, 0, 1, 1, 1, 1, 0.0)
        self.device = torch.device(device)
        self.cuda = self.device.type == "cuda"
        self.prefetch, self.seed, self.drop_last = max(1, int(prefetch)), int(seed), drop_last
        self.cpad, self.s2d, self.return_index = cpad, Fn.s2d_for(s2d, self.out_size, self.out_size), return_index
        self.mean = torch.tensor(mean, dtype=torch.float32, device=self.device)
        self.std = torch.tensor(std, dtype=torch.float32, device=self.device)
        self.epoch = 0
        self.resample, self.tap = resample, None
        exact = resample == "pil" and self.aug.mode != MODE_PADCROP
        stride = int(self.gather.hdr["max_bytes"])
        pin = self.cuda
        nslots = self.prefetch + 1
        self.slots = [dict(buf=torch.empty(self.batch_size * stride, dtype=torch.uint8, pin_memory=pin),
                           meta=torch.empty((self.batch_size, 8), dtype=torch.int64, pin_memory=pin),
                           labels=torch.empty(self.batch_size, dtype=torch.int64, pin_memory=pin),
                           xf=(torch.empty((self.batch_size, 8), dtype=torch.float32, pin_memory=pin)
                               if self.aug.affine and not exact else None),
                           geo=(torch.empty((self.batch_size, 12), dtype=torch.int32, pin_memory=pin)
                                if exact else None),
                           idx=None, event=None) for _ in range(nslots)]
        self.stream = torch.cuda.Stream(device=self.device) if self.cuda else None

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)
        if self.sampler is not None and hasattr(self.sampler, "set_epoch"):
            self.sampler.set_epoch(epoch)

    def _order(self):
        if self.sampler is None:
            return list(range(len(self.gather)))
        return list(iter(self.sampler))

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.gather)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def _batches(self):
        order = self._order()
        nb = len(self)
        for i in range(nb):
            yield torch.tensor(order[i * self.batch_size:(i + 1) * self.batch_size], dtype=torch.int64)

    def _submit(self, slot, idx):
        if slot["event"] is not None:
            slot["event"].synchronize()  # the previous H2D copy out of this slot has finished
            slot["event"] = None
        B = idx.numel()
        slot["idx"] = idx
        epoch = getattr(self.sampler, "epoch", self.epoch)  # the training loop drives sampler.set_epoch
        xf = slot["xf"][:B] if slot["xf"] is not None else None
        geo = slot["geo"][:B] if slot["geo"] is not None else None
        slot["ticket"] = self.gather.submit(idx, slot["buf"], slot["meta"][:B], slot["labels"][:B], self.aug,
                                            self.seed, epoch, xf, (self.out_size, self.out_size), geo)

    def _convert(self, slot):
        """Join the host gather of ``slot`` and run H2D + augment + normalise (side stream)."""
        self.gather.wait(slot["ticket"])
        idx = slot["idx"]
        B = idx.numel()
        meta = slot["meta"][:B]
        used = int(meta[:, 0].max().item()) + int((meta[:, 1] * meta[:, 2]).max().item()) * 3 if B else 0
        used = min(used, slot["buf"].numel())
        src = slot["buf"][:used].to(self.device, non_blocking=True)
        labels = slot["labels"][:B].to(self.device, non_blocking=True)
        if slot["geo"] is not None:
            extra = slot["geo"][:B]
            imgs = Fn.resample_exact(src, meta, extra, self.out_size, self.out_size, bicubic=self.aug.filter == 1)
        elif slot["xf"] is not None:
            extra = slot["xf"][:B]
            imgs = Fn.warp_crop(src, meta, extra, self.out_size, self.out_size)
        else:
            extra = None
            imgs = Fn.crop_resize(src, meta, self.out_size, self.out_size)
        if self.tap is not None:
            self.tap(imgs, meta, extra)
        plan = None
        if self.mix is not None:
            # Mixup / CutMix on the final uint8 batch, after crop / warp / resample (tap saw it unmixed)
            epoch = getattr(self.sampler, "epoch", self.epoch)
            plan = self.mix.device_plan(B, self.out_size, self.out_size, slot["step"], self.device, epoch=epoch)
        x = Fn.to_device_nhwc(imgs, self.mean, self.std, cpad=self.cpad, nchw=False, in_scale=1.0 / 255.0,
                              s2d=self.s2d, mix=plan)
        out = (x, labels) if plan is None else (x, labels, plan.partner, plan.wlab)
        if self.return_index:
            out = out + (idx.to(self.device, non_blocking=True),)
        if self.cuda:
            slot["event"] = torch.cuda.Event()
            slot["event"].record(self.stream)
        else:
            out = tuple(t.clone() for t in out)  # CPU: detach from the reusable slot buffers
        return out

    def __iter__(self):
        batches = enumerate(self._batches())
        inflight = deque()
        free = deque(self.slots)

        def fill():
            while free and len(inflight) < self.prefetch:
                try:
                    step, idx = next(batches)
                except StopIteration:
                    return
                s = free.popleft()
                s["step"] = step  # the batch's position in the epoch: the mix plan is a function of it
                self._submit(s, idx)
                inflight.append(s)

        fill()
        cur_stream = torch.cuda.current_stream(self.device) if self.cuda else None
        try:
            while inflight:
                s = inflight.popleft()
                if self.cuda:
                    with torch.cuda.stream(self.stream):
                        out = self._convert(s)
                    cur_stream.wait_stream(self.stream)
                    for t in out:
                        t.record_stream(cur_stream)
                else:
                    out = self._convert(s)
                free.append(s)
                fill()
                yield out
        finally:
            # an abandoned epoch (break / exception) must not leave host threads writing into
            # slots that the next epoch, or the allocator, hands out again
            for s in inflight:
                try:
                    self.gather.wait(s["ticket"])
                except RuntimeError:
                    pass

    def close(self):
        self.gather.close()

    def __del__(self):
        try:
            self.close()  # joins the host threads while the pinned slots are still alive
        except Exception:
            pass
