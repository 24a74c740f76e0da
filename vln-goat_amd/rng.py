"""The dropout counter of the HIP kernels: every op that draws a mask takes its (seed, offset, device counter) from here."""
import torch


class RngState:
    """Dropout counter state.  Eager: host counter.  Graph capture: `dev` (uint64 on device) is bumped
    by one in-graph add per replay so every replay draws fresh masks (see goat_hip.h).  `dev` is process-wide: once set, EVERY op adds
    its value to the seed, so whoever sets it owns the random streams of the process.  Code that needs a counter of its own for a graph
    (speaker.IncrementalDecoder) installs it around its own ops only and puts the previous value back."""
    seed = None         # None: taken from torch.initial_seed() at first use (so torch.manual_seed / the reference trainer's
    rank_salt = 0       # set_random_seed(seed + rank) steer it); rank_salt: GoatDataParallel folds the rank in
    base = None         # what manual_seed() was given
    counter = 0
    dev = None

    @classmethod
    def next(cls, numel):
        if cls.seed is None:
            cls.seed = (int(torch.initial_seed()) * 0x9E3779B97F4A7C15 + 0x5EED + cls.rank_salt * 0xD1B54A32D192ED03) & 0x7FFFFFFFFFFFFFFF
        off = cls.counter
        cls.counter += (int(numel) + 7) & ~7      # multiples of 8: row kernels draw masks per even-aligned counter pair
        return cls.seed, off, (cls.dev.data_ptr() if cls.dev is not None else None)

    @classmethod
    def draw(cls, p, numel):
        """next(numel) for an op that drops with probability p; p <= 0 draws nothing and consumes nothing: (0, 0, None)."""
        return cls.next(numel) if p > 0 else (0, 0, None)


def manual_seed(seed=None):
    """Seed of the dropout masks of the HIP kernels.  None: re-derive from torch.initial_seed() (call after torch.manual_seed)."""
    RngState.base = seed
    RngState.seed = None if seed is None else (int(seed) + RngState.rank_salt * 0xD1B54A32D192ED03) & 0x7FFFFFFFFFFFFFFF
    RngState.counter = 0
