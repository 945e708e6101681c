"""The reference's per-iteration scalars (audiogan.py:776-809 for a critic iteration, :875-884, :911-920, :940 for a generator
iteration) kept on the device: ``train.d_step_full / g_step_full(summary=...)`` compute the statistics with library kernels
and gather them with ONE launch into a row of a ring (``kernels.summary_commit``); the host reads the ring in one copy
whenever it wants (``Summary.drain``).  No host read is added to an iteration, so captured iterations log like eager ones.

A drain is also the run's health check: every row carries the optimiser's NaN / |g| > 1e5 flags (``check_grad``,
audiogan.py:232-240, which the reference asserts on every iteration, :786, :909) and the sticky status word of the
persistent recurrent launches; ``drain`` raises what ``optim._Fused.step(check=True)`` raises.

Row layout (16 words; integers stored as int32 bits):
    col   critic iteration ('D')          generator iteration ('G')
    0     kind = 0                        kind = 1
    1     sequence number (written by the commit launch)
    2     loss_d                          bce  (the ``_loss`` of :940)
    3     loss_g                          feature_penalty
    4     loss                            loss
    5     cls_d/mean                      reward/mean
    6     cls_d/std                       reward/std
    7     cls_g/mean                      reward_baseline
    8     cls_g/std                       g_grad_norm
    9     acc_d                           lambda_fp
    10    acc_g                           -
    11    d_grad_norm                     -
    12    x_grad_norm                     -
    13    optimiser flags (bit 0: NaN, bit 1: |g| > 1e5)
    14    sticky status word of the persistent workspace
    15    -
"""
import json

import numpy as np
import torch

from . import kernels as K

KIND_D, KIND_G = 0, 1
COLS = K.SUMMARY_COLS
COL_FLAGS, COL_STICKY = 13, 14
D_TAGS = ('loss_d', 'loss_g', 'loss', 'cls_d/mean', 'cls_d/std', 'cls_g/mean', 'cls_g/std', 'acc_d', 'acc_g', 'd_grad_norm',
          'x_grad_norm')
G_TAGS = ('bce', 'feature_penalty', 'loss', 'reward/mean', 'reward/std', 'reward_baseline', 'g_grad_norm', 'lambda_fp')


class Summary(object):
    def __init__(self, device, capacity=256, on_row=None, path=None):
        """``capacity``: rows of the ring; ``on_row(row)``: called with every drained row (a dict: the reference's tag names
        plus ``kind`` 'D' / 'G', ``iter``, ``bce``, ``lambda_fp``) - the hook for a TensorBoard writer; ``path``: every
        drained row is appended there as one JSON line."""
        assert capacity >= 1
        self.dev, self.capacity, self.on_row, self.path = torch.device(device), int(capacity), on_row, path
        # the cursor (next row, next sequence number) lives behind the ring: one copy brings both to the host
        self._buf = torch.zeros((self.capacity + 1) * COLS, dtype=torch.int32, device=self.dev)
        self.ring = self._buf[:self.capacity * COLS].view(self.capacity, COLS)
        self.cursor = self._buf[self.capacity * COLS:self.capacity * COLS + 2]
        self.pending = []            # (kind, iteration) of every committed row not drained yet, oldest first
        self._seq = 0                # sequence number of pending[0]
        self._count = {KIND_D: 0, KIND_G: 0}
        # where the statistics kernels of an iteration leave their results (stable addresses: a captured iteration's
        # commit reads the same words on every replay)
        self.stat_d = torch.zeros(5, device=self.dev)
        self.stat_g = torch.zeros(5, device=self.dev)
        self.stat_r = torch.zeros(2, device=self.dev)
        self._parts = {}

    def part(self, n):
        """[n] fp32 scratch for the per-clip input-gradient norms"""
        p = self._parts.get(n)
        if p is None:
            p = self._parts[n] = torch.zeros(n, device=self.dev)
        return p

    # ---- the iteration's side ---------------------------------------------------------------------------
    def _capturing(self):
        return self.dev.type == 'cuda' and torch.cuda.is_current_stream_capturing()

    def expect(self, kind, iteration=None):
        """one more row is about to be committed (by an iteration or by the replay of a captured one): a full ring is
        drained first, so no row is ever overwritten unseen"""
        if len(self.pending) >= self.capacity:
            self.drain()
        self._count[kind] += 1
        self.pending.append((kind, self._count[kind] if iteration is None else int(iteration)))

    def commit(self, kind, iteration, cols, part=None, part_col=-1):
        """gather the iteration's device scalars into the next row (one launch).  ``cols``: {column: one-element device
        tensor | float | int}.  Under hipGraph capture nothing executes: the row is expected when the graph is replayed
        (``expect``)."""
        if not self._capturing():
            self.expect(kind, iteration)
        row = [None] * COLS
        row[0] = int(kind)
        for c, v in cols.items():
            row[c] = v
        row[COL_STICKY] = K.persist_status_word(self.dev) if self.dev.type == 'cuda' else None
        K.summary_commit(self.ring, self.cursor, row, part=part, part_col=part_col)

    # ---- the host's side --------------------------------------------------------------------------------
    @staticmethod
    def _row(kind, iteration, w):
        f = w.view(np.float32)
        tags = D_TAGS if kind == KIND_D else G_TAGS
        r = dict(kind='D' if kind == KIND_D else 'G', iter=iteration)
        for i, t in enumerate(tags):
            r[t] = float(f[2 + i])
        return r

    def drain(self):
        """one D2H copy of ring + cursor -> the rows committed since the last drain, oldest first (dicts), each handed to
        ``on_row`` and appended to ``path``.  Raises on the first row whose optimiser flags or persistent status word report
        a bad iteration - the exceptions of ``optim._Fused.step(check=True)``; rows in front of it are delivered."""
        if not self.pending:
            return []
        host = self._buf.cpu().numpy()         # (a copy on the current stream: every enqueued commit has run)
        ring, cur = host[:self.capacity * COLS].reshape(self.capacity, COLS), host[self.capacity * COLS:]
        pend, seq0 = self.pending, self._seq
        self.pending, self._seq = [], seq0 + len(pend)
        if int(cur[1]) != seq0 + len(pend) or len(pend) > self.capacity:
            raise RuntimeError('Summary.drain: the device committed %d rows since the last drain, the host expected %d '
                               '(ring of %d rows): rows were lost' % (int(cur[1]) - seq0, len(pend), self.capacity))
        out = []
        fh = open(self.path, 'a') if self.path is not None else None
        try:
            for k, (kind, it) in enumerate(pend):
                w = ring[(seq0 + k) % self.capacity]
                if int(w[1]) != seq0 + k or int(w[0]) != kind:
                    raise RuntimeError('Summary.drain: row %d holds (kind %d, sequence %d), expected (%d, %d)'
                                       % ((seq0 + k) % self.capacity, int(w[0]), int(w[1]), kind, seq0 + k))
                flags, sticky = int(w[COL_FLAGS]), int(w[COL_STICKY]) & 0xFFFFFFFF
                if sticky:
                    K.lstm_persist_status(self.dev, reset=True)
                    raise K.PersistentLaunchError(K.persist_error_text(sticky))
                assert not (flags & 1), 'NaN in gradients (check_grad)'
                assert not (flags & 2), '|grad| > 1e5 (check_grad)'
                r = self._row(kind, it, w)
                if self.on_row is not None:
                    self.on_row(r)
                if fh is not None:
                    fh.write(json.dumps(r) + '\n')
                out.append(r)
        finally:
            if fh is not None:
                fh.close()
        return out
