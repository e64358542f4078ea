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


class SyntheticMaskedLM(torch.utils.data.Dataset):
    """Synthetic masked-language-model data for BERT pre-training: ``(ids [S], labels [S])`` per row.

    Learnable text: row i is the arithmetic progression ``5 + (a_i + t * d_i) mod (vocab_size - 5)`` with
    ``d_i`` in {1, 2, 3}, so a masked token follows from its neighbours. Static BERT masking, made once
    from the seed: ``k_i = min(P, max(1, round(mask_prob * len_i)))`` distinct positions among the real
    tokens (``P`` = ``max_predictions``, default ceil(mask_prob * S) rounded up to 8); 80 % of them become
    ``mask_id``, 10 % a random id >= 5, 10 % keep their token. ``labels`` hold the original id at those
    positions and -100 elsewhere. With ``min_len`` the rows are variable-length (lengths uniform in
    ``[min_len, seq_len]``) and right-padded with ``pad_id``; pads are never chosen. ``lengths`` holds the
    row lengths, ``original`` the unmasked ids."""

    def __init__(self, n: int, seq_len: int = 512, vocab_size: int = 30522, mask_prob: float = 0.15,
                 max_predictions=None, mask_id: int = 4, seed: int = 0, min_len=None, pad_id: int = 0):
        if vocab_size <= 8:
            raise ValueError("vocab_size must exceed 8 (ids below 5 are reserved)")
        if not 0.0 < mask_prob < 1.0:
            raise ValueError(f"mask_prob must satisfy 0 < p < 1, got {mask_prob}")
        from ml_trainer_amd.ops.mlm import default_max_predictions
        P = default_max_predictions(seq_len, mask_prob) if max_predictions is None else int(max_predictions)
        if P < 1:
            raise ValueError(f"max_predictions must be >= 1, got {P}")
        rng = np.random.default_rng(seed)
        a = rng.integers(0, vocab_size - 5, size=(n, 1), dtype=np.int64)
        d = rng.integers(1, 4, size=(n, 1), dtype=np.int64)
        t = np.arange(seq_len, dtype=np.int64)[None, :]
        original = 5 + (a + t * d) % (vocab_size - 5)
        lengths = np.full(n, seq_len, dtype=np.int64)
        if min_len is not None:
            if not 1 <= min_len <= seq_len:
                raise ValueError(f"min_len must satisfy 1 <= min_len <= seq_len = {seq_len}, got {min_len}")
            lengths = rng.integers(min_len, seq_len + 1, size=n, dtype=np.int64)
        pad = t >= lengths[:, None]
        original[pad] = pad_id
        k = np.minimum(P, np.maximum(1, np.rint(mask_prob * lengths).astype(np.int64)))
        k = np.minimum(k, lengths)
        keys = rng.random((n, seq_len))
        keys[pad] = 2.0  # pads sort last: never among the first k_i <= len_i
        order = np.argsort(keys, axis=1, kind="stable")
        rank = np.empty_like(order)
        np.put_along_axis(rank, order, np.broadcast_to(t, order.shape), axis=1)
        chosen = rank < k[:, None]
        u = rng.random((n, seq_len))
        rand_ids = rng.integers(5, vocab_size, size=(n, seq_len), dtype=np.int64)
        ids = original.copy()
        ids[chosen & (u < 0.8)] = mask_id
        swap = chosen & (u >= 0.8) & (u < 0.9)
        ids[swap] = rand_ids[swap]
        labels = np.where(chosen, original, -100)
        self.ids = torch.from_numpy(ids)
        self.labels = torch.from_numpy(labels)
        self.original = torch.from_numpy(original)
        self.lengths = torch.from_numpy(lengths)
        self.seq_len, self.max_predictions, self.mask_id = seq_len, P, mask_id
        self.pad_id = pad_id if min_len is not None else None

    def __len__(self) -> int:
        return self.ids.shape[0]

    def __getitem__(self, i):
        return self.ids[i], self.labels[i]


class SyntheticCausalLM(torch.utils.data.Dataset):
    """Synthetic next-token data for the causal language-model task: ``(ids [S], labels [S])`` per row.

    The rows are ``SyntheticMaskedLM``'s arithmetic progressions ``5 + (a_i + t * d_i) mod (vocab_size - 5)``,
    unmasked. With ``d_i`` in {1, 2, 3} the next token follows from the two before it (their difference is
    the step), so the task needs attention and is learnable. ``labels`` are already shifted:
    ``labels[s] = ids[s + 1]`` where ``s + 1 < len_i``, and -100 at each row's last real token and at the
    pads. With ``min_len`` the rows are variable-length (lengths uniform in ``[min_len, seq_len]``) and
    right-padded with ``pad_id``. ``lengths`` holds the row lengths."""

    def __init__(self, n: int, seq_len: int = 512, vocab_size: int = 30522, seed: int = 0, min_len=None,
                 pad_id: int = 0):
        if vocab_size <= 8:
            raise ValueError("vocab_size must exceed 8 (ids below 5 are reserved)")
        rng = np.random.default_rng(seed)
        a = rng.integers(0, vocab_size - 5, size=(n, 1), dtype=np.int64)
        d = rng.integers(1, 4, size=(n, 1), dtype=np.int64)
        t = np.arange(seq_len, dtype=np.int64)[None, :]
        ids = 5 + (a + t * d) % (vocab_size - 5)
        lengths = np.full(n, seq_len, dtype=np.int64)
        if min_len is not None:
            if not 1 <= min_len <= seq_len:
                raise ValueError(f"min_len must satisfy 1 <= min_len <= seq_len = {seq_len}, got {min_len}")
            lengths = rng.integers(min_len, seq_len + 1, size=n, dtype=np.int64)
        labels = np.full_like(ids, -100)
        labels[:, :-1] = ids[:, 1:]
        labels[t + 1 >= lengths[:, None]] = -100
        ids[t >= lengths[:, None]] = pad_id
        self.ids = torch.from_numpy(ids)
        self.labels = torch.from_numpy(labels)
        self.lengths = torch.from_numpy(lengths)
        self.seq_len = seq_len
        self.pad_id = pad_id if min_len is not None else None

    def __len__(self) -> int:
        return self.ids.shape[0]

    def __getitem__(self, i):
        return self.ids[i], self.labels[i]
