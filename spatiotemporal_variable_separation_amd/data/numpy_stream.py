"""A NumPy random stream that lives on the device: `DeviceRandomState` holds the MT19937 state of an `np.random.RandomState` in HBM and
draws tables of scalar `randint(low, high)` values from it with one launch (ops.mt19937_randint, csrc/vs_mt19937.hip), bit for bit the
values the host stream gives for the same calls in the same order.  The Moving-MNIST training loader uses it for its five draws per
digit (data/moving_mnist.py), which leaves no draw, upload or synchronisation on the host per batch.

Only the scalar `randint` of the legacy stream is provided.  The Gaussian cache of the source (`has_gauss`, `cached_gaussian`) is carried
along unchanged, so that a state handed back to the host continues every distribution where the source would."""
import numpy as np
import torch

from .. import ops
from .._lib import VarsepHipError

_N = 624


class DeviceRandomState:
    """`DeviceRandomState(source, device)`: `source` is an `np.random.RandomState`, whose state is copied (the source itself is not
    advanced by this object afterwards: the two are separate streams that start at the same point), or None for a snapshot of the global
    NumPy stream, which is left as it is.  Launches go to the current HIP stream; they continue the sequence in launch order."""

    def __init__(self, source=None, device='cuda'):
        state = (np.random if source is None else source).get_state()
        name, key, pos = state[0], np.asarray(state[1], dtype=np.uint32), int(state[2])
        if name != 'MT19937' or key.shape != (_N,) or not 0 <= pos <= _N:
            raise VarsepHipError('DeviceRandomState: an MT19937 state with 624 key words and 0 <= pos <= 624 expected (got %r, %s words, '
                                 'pos %d)' % (name, key.shape, pos))
        self._gauss = (int(state[3]), float(state[4]))
        self.device = torch.device(device)
        words = np.concatenate([key, np.array([pos], dtype=np.uint32)])
        self.state = torch.from_numpy(words.view(np.int32)).to(self.device)

    def randint_table(self, lows, highs, n_rows):
        """int32 [n_rows, k] on the device: entry (r, j) is the (r * k + j)-th scalar `randint(lows[j], highs[j])` of the stream.  One
        launch; nothing is read back (the state was checked when it was uploaded)."""
        return ops.mt19937_randint(self.state, lows, highs, n_rows, validate=False)

    def stochastic_trajectories(self, n_traj, seq_len, lows, highs, x_max, y_max, max_speed, **kwargs):
        """(pre, positions, latents, desc) of `n_traj` stochastic Moving-MNIST trajectories drawn from the stream (ops.mmnist_stochastic_
        trajectories, which documents the operands).  One launch; nothing is read back."""
        return ops.mmnist_stochastic_trajectories(self.state, n_traj, seq_len, lows, highs, x_max, y_max, max_speed, validate=False, **kwargs)

    def get_state(self):
        """NumPy's state tuple ('MT19937', key, pos, has_gauss, cached_gaussian) of the stream as it stands after the launches enqueued
        so far (a download: it waits for them).  The stream itself stays where it is."""
        words = self.state.cpu().numpy().view(np.uint32)
        return ('MT19937', words[:_N].copy(), int(words[_N]), self._gauss[0], self._gauss[1])

    def to_random_state(self):
        """A host `np.random.RandomState` at the same point of the stream."""
        rs = np.random.RandomState(0)
        rs.set_state(self.get_state())
        return rs
