"""GPU: what the HBM-resident datasets share (data/device.py) -- `TimelineSet` on a 40-frame timeline, read forwards and backwards, against
a NumPy gather, and one shuffled epoch of `DeviceBatchLoader` against torch's own samplers."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F, SEQ_LEN, NT_COND = 40, 5, 2


def _table(step):
    """Windows valid for `step`; entries 0 and 1 touch frame 0 and frame F - 1 -- as first and as last frame of a window."""
    if step == 1:
        return np.array([0, F - SEQ_LEN, 5, 17, 11, F - SEQ_LEN - 1, 1, 20, 3], dtype=np.int32)
    return np.array([F - 1, SEQ_LEN - 1, 17, 30, SEQ_LEN, F - 2, 12, 25, 9], dtype=np.int32)


def _case(frame_elems, step):
    """(the set on the device, its windows fp32 [N, SEQ_LEN, 2, frame_elems / 2] gathered by NumPy).  No zero value in the timeline: a
    zeroed row would be recognisable."""
    from spatiotemporal_variable_separation_amd.data.device import TimelineSet
    frames = np.random.RandomState(1000 + frame_elems).uniform(0.5, 2.0, size=(F, frame_elems)).astype(np.float32)
    first = _table(step)
    rows = first.astype(np.int64)[:, None] + step * np.arange(SEQ_LEN)[None]
    assert rows.min() == 0 and rows.max() == F - 1 and (rows[0, 0], rows[1, -1]) == ((0, F - 1) if step == 1 else (F - 1, 0))
    shape = (2, frame_elems // 2)
    ds = TimelineSet(torch.from_numpy(frames).cuda(), torch.from_numpy(first).cuda(), SEQ_LEN, NT_COND, shape)
    ds.step = step
    return ds, torch.from_numpy(frames[rows].reshape((len(first), SEQ_LEN) + shape))


@pytest.mark.parametrize('step', [1, -1])
@pytest.mark.parametrize('frame_elems', [12, 2048])
def test_timeline_set_matches_numpy(frame_elems, step):
    from spatiotemporal_variable_separation_amd._lib import VarsepHipError
    ds, ref = _case(frame_elems, step)
    n = len(ds)
    assert n == len(ref) == 9 and ds.device_resident
    items = [1, 0, 8, 3, 3, 5, 7]
    for idx in (items, torch.tensor(items, dtype=torch.int32).cuda()):
        cond, target = ds.batch(idx)
        assert tuple(cond.shape) == (7, NT_COND, 2, frame_elems // 2) and tuple(target.shape) == (7, SEQ_LEN - NT_COND, 2, frame_elems // 2)
        got = torch.cat([cond, target], dim=1).cpu()
        assert got.dtype == torch.float32 and np.array_equal(got.numpy().view(np.uint32), ref[items].numpy().view(np.uint32))
        c16, t16 = ds.batch(idx, torch.bfloat16)
        assert c16.dtype == torch.bfloat16 and torch.equal(torch.cat([c16, t16], dim=1).cpu(), ref[items].to(torch.bfloat16))
    for i in (0, 1, n - 1):
        item, (cb, tb) = ds[i], ds.batch([i])
        assert len(item) == 2 and torch.equal(item[0], cb[0]) and torch.equal(item[1], tb[0])
        assert torch.equal(torch.cat(item).cpu(), ref[i])
    for bad in ([n], [0, -1], []):
        with pytest.raises(IndexError):
            ds.batch(bad)
    with pytest.raises(VarsepHipError):
        ds.batch(torch.tensor([0, n], dtype=torch.int32).cuda())


def test_device_loader_visits_the_dataloader_items():
    """DeviceBatchLoader under a fixed torch.manual_seed yields the items `DataLoader(shuffle=True)` would: a DataLoader iterator draws its
    base seed, then its RandomSampler draws the permutation.  9 windows in batches of 4: a ragged last batch of 1."""
    from torch.utils.data import BatchSampler, RandomSampler
    from spatiotemporal_variable_separation_amd.data.device import DeviceBatchLoader
    ds, ref = _case(12, -1)
    torch.manual_seed(17)
    torch.empty((), dtype=torch.int64).random_()          # _BaseDataLoaderIter.__init__: the base seed
    want = list(BatchSampler(RandomSampler(ds), 4, False))
    assert sorted(i for b in want for i in b) == list(range(9)) and [len(b) for b in want] == [4, 4, 1]
    torch.manual_seed(17)
    got = list(DeviceBatchLoader(ds, 4, shuffle=True))
    assert len(got) == len(want)
    for (cond, target), items in zip(got, want):
        assert torch.equal(torch.cat([cond, target], dim=1).cpu(), ref[items])
