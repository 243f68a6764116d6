"""What the HBM-resident datasets share: the device check, the batch loader, the one-item form of a batch, the timeline set (an fp32
[F, elems] timeline plus an int32 table of first frames: TaxiBJ read backwards, SST read forwards) and the optional file reader."""
import importlib
import os

import numpy as np
import torch
from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler

from .. import ops
from .._lib import VarsepHipError


def require_gpu(what, device, hint=''):
    """torch.device of `device` (None: cuda); VarsepHipError when it is not a GPU -- no dataset here has a host path."""
    device = torch.device(device if device is not None else 'cuda')
    if device.type != 'cuda':
        raise VarsepHipError('the HBM-resident %s set needs an MI355X device; there is no CPU fallback%s' % (what, hint))
    return device


def optional_module(name):
    """The module `name` (h5py, netCDF4, PIL.Image) when it imports, else None.  Imported per call: a module that appears later is found."""
    try:
        return importlib.import_module(name)
    except ImportError:
        return None


def read_optional(module_name, native_path, npz_path, read_native, read_npz, unit, hint):
    """`read_native(module, native_path)` when `module_name` imports and the native file exists, else `read_npz(z)` of the opened .npz
    file, else ValueError saying which of the two conditions failed and how to convert (`hint`) each `unit` (year, zone)."""
    module = optional_module(module_name)
    if module is not None and os.path.isfile(native_path):
        return read_native(module, native_path)
    if os.path.isfile(npz_path):
        with np.load(npz_path) as z:
            return read_npz(z)
    why = 'is missing' if not os.path.isfile(native_path) else 'cannot be read: %s does not import here' % module_name
    raise ValueError('%s %s, and there is no %s.  Where %s exists, convert each %s with\n%s'
                     % (native_path, why, npz_path, module_name, unit, hint))


class DeviceSet:
    """A set whose `batch(item_idx, out_dtype)` assembles (cond, target, ...) on the device; an item is row 0 of a batch of one."""

    device_resident = True

    def __getitem__(self, index):
        return tuple(t[0] for t in self.batch([int(index)]))


class TimelineSet(DeviceSet):
    """Windows of `seq_len` frames out of `frames` fp32 [F, elems] on the device: window i starts at frame `first[i]` (int32 [N] on the
    device) and advances by `step` (+1 or -1) frames per position.  Items are (cond [nt_cond, *frame_shape], target [seq_len - nt_cond,
    *frame_shape])."""

    step = None                                          # set by the subclass

    def __init__(self, frames, first, seq_len, nt_cond, frame_shape):
        self.frames, self.first = frames, first
        self.seq_len, self.nt_cond, self.frame_shape = seq_len, nt_cond, tuple(frame_shape)

    def __len__(self):
        return self.first.numel()

    def _device_index(self, item_idx):
        """(int32 device tensor [B], whether the kernel must check it): a host list is range-checked here (IndexError) and uploaded, a
        device tensor goes to the kernel as it is and is checked there."""
        if isinstance(item_idx, torch.Tensor):
            return item_idx, True
        idx = np.asarray(list(item_idx), dtype=np.int64).reshape(-1)
        if idx.size == 0 or idx.min() < 0 or idx.max() >= len(self):
            raise IndexError('an item index is outside the %d windows of the set' % len(self))
        return torch.from_numpy(idx.astype(np.int32)).to(self.frames.device, non_blocking=True), False

    def _gather(self, item_idx, validate, out_dtype):
        x = ops.gather_timeline(self.frames, self.first, item_idx, self.seq_len, self.step, out_dtype, validate=validate)
        x = x.view((x.shape[0], self.seq_len) + self.frame_shape)
        return x[:, :self.nt_cond], x[:, self.nt_cond:]

    def batch(self, item_idx, out_dtype=torch.float32):
        """item_idx: list of ints or an int32 device tensor [B] -> (cond [B, nt_cond, ...], target [B, seq_len - nt_cond, ...]), one launch."""
        return self._gather(*self._device_index(item_idx), out_dtype)


class DeviceBatchLoader:
    """`DataLoader(dataset, batch_size, shuffle=True)` of main.py:113 for a device-resident set: same sampler classes (so the
    same seeded index stream and the same ragged last batch), batches gathered by one launch instead of worker processes."""

    def __init__(self, dataset, batch_size, shuffle=True, drop_last=False, sampler=None, generator=None, out_dtype=torch.float32):
        assert getattr(dataset, 'device_resident', False), 'DeviceBatchLoader serves HBM-resident datasets'
        self.dataset, self.batch_size, self.drop_last, self.out_dtype = dataset, batch_size, drop_last, out_dtype
        if sampler is None:
            sampler = RandomSampler(dataset, generator=generator) if shuffle else SequentialSampler(dataset)
        self.sampler, self.generator = sampler, generator
        self.batch_sampler = BatchSampler(sampler, batch_size, drop_last)

    def __len__(self):
        return len(self.batch_sampler)

    def __iter__(self):
        # a DataLoader iterator draws its base seed from the RNG before the sampler draws its own (torch/utils/data/dataloader.py,
        # _BaseDataLoaderIter.__init__); consume the same draw so that a seeded epoch visits the same items
        torch.empty((), dtype=torch.int64).random_(generator=self.generator)
        for items in self.batch_sampler:
            yield self.dataset.batch(items, self.out_dtype)
