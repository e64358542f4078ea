"""Synthetic sequence-classification data for the BERT configs (no network: no
GLUE download). Token ids uniform over the vocabulary (ids >= 5 so special ids
stay free); with ``learnable=True`` the label is decided by whether a marker
token appears in the first half of the sequence, so training curves move.

With ``min_len`` the rows are variable-length and right-padded: each row's length is drawn uniformly
from ``[min_len, seq_len]`` (from the same seeded generator, after every other draw, so the tokens and
labels of the fixed-length dataset are unchanged), the positions past it hold ``pad_id`` and the
marker is moved inside the sequence. ``lengths`` holds the row lengths."""
from __future__ import annotations

import numpy as np
import torch


class SyntheticTextClassification(torch.utils.data.Dataset):
    def __init__(self, n: int, seq_len: int = 512, vocab_size: int = 30522, num_labels: int = 2, seed: int = 0,
                 learnable: bool = False, min_len=None, pad_id: int = 0):
        rng = np.random.default_rng(seed)
        self.ids = torch.from_numpy(rng.integers(5, vocab_size, size=(n, seq_len), dtype=np.int64))
        self.targets = torch.from_numpy(rng.integers(0, num_labels, size=n, dtype=np.int64))
        pos = torch.from_numpy(rng.integers(1, max(seq_len // 2, 2), size=n)) if learnable else None
        self.lengths = torch.full((n,), seq_len, dtype=torch.int64)
        if min_len is not None:
            if not 1 <= min_len <= seq_len:
                raise ValueError(f"min_len must satisfy 1 <= min_len <= seq_len = {seq_len}, got {min_len}")
            self.lengths = torch.from_numpy(rng.integers(min_len, seq_len + 1, size=n, dtype=np.int64))
            self.ids[torch.arange(seq_len)[None, :] >= self.lengths[:, None]] = pad_id
            if learnable:
                pos = torch.minimum(pos, self.lengths - 1)  # the marker lands inside the sequence
        if learnable:
            marker = 3
            has = self.targets == 1
            self.ids[has, pos[has]] = marker
        self.classes = [str(i) for i in range(num_labels)]
        self.seq_len = seq_len
        self.pad_id = pad_id if min_len is not None else None

    def __len__(self) -> int:
        return self.ids.shape[0]

    def __getitem__(self, i):
        return self.ids[i], int(self.targets[i])
