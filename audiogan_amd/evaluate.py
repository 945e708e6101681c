"""Held-out evaluation: how the critic scores clips it was never trained on, and how far the generator's samples are from
real audio in their long-term average spectrum.

The reference keeps a validation loader beside the training one (``dataset.dataloader``; audiogan.py:672 draws its fixed
sample words from it) and never scores it: every number it logs is measured on the minibatch just trained on.  ``Evaluator``
adds the pass.  With up to 100 critic iterations per generator iteration, the critic's accuracy on unseen clips is the
diagnostic for that schedule; the spectral distance is a number where there were only WAV files to listen to.

The held-out set is FIXED when the evaluator is built: ``batches`` minibatches are taken from ``heldout`` once, padded to the
frame grid as ``TrainLoop._real`` pads, and kept on the device with their lengths and words; one z and one tensor of stop
uniforms per minibatch come from a private ``torch.Generator(seed)``.  ``dataset.py`` draws from the GLOBAL numpy generator,
so a validation ``next()`` in the middle of training would move the training data order: a caller who passes a loader builds
the evaluator BEFORE the training loader's first ``next()`` (the reference takes its validation batch at :672 the same way),
or passes a list of minibatches taken earlier.  After construction a pass draws nothing from the global torch, CUDA or numpy
generators and leaves ``.grad``, the optimiser state and the loaders alone: it changes no training bit.

What a pass measures (``run``), per held-out minibatch, without instance noise and under ``torch.no_grad()``:

    real clips     d(real, len, e_d(words))                -> loss_d, acc_d, cls_d/mean, cls_d/std     (BCE towards 0.9)
    fakes          g.generate(e_g(words), z_i, u_i), d(..) -> loss_g, acc_g, cls_g/mean, cls_g/std     (BCE towards 0)
    both           feature_penalty_fused of the two sets of conv activations      -> feature_penalty (mean over minibatches)
    spectrum       ltas_power(fake) against the real clips' (computed once)       -> ltas_db
    aligned=True   dtw_cost(melcep_frames(fake), melcep_frames(real), computed once)  -> mcd_db
    crossed=True   dtw_pairs(every fake's cepstra x every real clip's of the minibatch)  -> nn_db, cover_db, word_hit
    draws=k        k - 1 further fakes per word, dtw_pairs between the draws             -> div_db (beside real_div_db)
    pitch=True     pitch_frames(fake), dtw_align instead of dtw_cost, pitch_path_accum   -> f0_rmse_cents, vuv_err, gpe

``ltas_db`` is the mean over all clips of sqrt(mean_k (dB_fake[k] - dB_real[k])^2), dB = 10 log10(P + 1e-10) over the 129 bins
of ``kernels.ltas_power``; fake i and real clip i share their word.  The statistics are accumulated on the device
(``kernels.score_accum``: means and deviations over VALID frames only, unlike the per-iteration summaries) in one small
float64 buffer that comes to the host in ONE copy per pass; the only other host reads are ``generate``'s own, one per
minibatch.

``mcd_db`` (off by default) is what ``ltas_db`` cannot see - the ORDER in which the energy moves through the bands.  Every
256-sample frame (hop 128) of a clip becomes 13 mel cepstra (24 triangular bands up to 4 kHz, natural logarithm, DCT-II:
``kernels.melcep_frames``); fake i and real clip i, which differ in length, are aligned by dynamic time warping over the
Euclidean distance d of cepstra 1..12 (c0, the level, is left out), symmetric steps D(i, j) = min(D(i-1, j) + d,
D(i, j-1) + d, D(i-1, j-1) + 2 d) (``kernels.dtw_cost``).  Every path from (0, 0) to (n-1, m-1) then has weight n + m, so
the total divided by n + m is a mean over the path that moves continuously with the inputs (dividing by the path's own
length would jump where two paths tie).  mcd_db = (10 / ln 10) sqrt(2) times the mean of that over all clips - the usual
mel-cepstral distortion in dB.  It is a distance between ONE fake and ONE real utterance of the word, not a perceptual
score: two real speakers of the same word are some dB apart as well, and only its trend over training says something.

``crossed`` and ``draws`` (both off by default, both need ``aligned``) ask the two questions one draw per word against one
real clip cannot answer.  ``crossed``: per held-out minibatch the aligned distance of EVERY fake to EVERY real clip, a [B, B]
matrix M in dB from one ``kernels.dtw_pairs`` launch (``crossed_scores`` states the rule).  ``nn_db`` is the mean over the
fakes of their nearest real clip's distance, ``cover_db`` the mean over the real clips of their nearest fake's - a
generator that says one word for every word keeps ``nn_db`` and loses ``cover_db``.  ``word_hit`` is the share of fakes
whose nearest real clip carries their own word, and ``word_hit/chance`` the share a blind guess would reach (the mean share
of the minibatch's real clips that carry the fake's word: 1 / B when all words differ).  This is retrieval among the B words of
one minibatch, to be read against ``word_hit/chance`` - not speech recognition.  ``draws=k``: k - 1 further (z, u) per
minibatch, drawn from the private generator AFTER every first draw (so those keep their bits), give k fakes per word;
``div_db`` is the mean aligned distance between two draws of the same word, over all clips and the k (k - 1) / 2 draw pairs.
Zero means z does nothing.  Two real utterances of a word are some dB apart as well, so ``div_db`` only means something
beside ``real_div_db``: the same mean over all pairs of held-out REAL clips that share a word, computed once when the
evaluator is built (None when no word occurs twice).  The extra fakes get no critic pass.

``pitch`` (off by default, needs ``aligned``) measures what the cepstra smooth away on purpose - the excitation.  13
coefficients from 24 bands of a 256-point frame carry no harmonics and c0 is left out, so a fake that is whispered where the
word is voiced, buzzes at one pitch or sits an octave off scores like a good one in ``mcd_db``.  ``kernels.pitch_frames``
gives every frame (the cepstra's own framing) a pitch candidate: the normalised cross-correlation of the 256-sample window
with its copy 19..128 samples later (400 Hz down to 63 Hz at 8 kHz), and of the local maxima within ``octf`` = 0.9 of the
largest the one at the SMALLEST lag, which is what avoids octave errors.  ``pitch_cents`` refines the lag by a parabola and
takes the logarithm, in float64: cents above 50 Hz, -1 where the frame is unvoiced (correlation below 0.5 or power below
1e-6).  ``kernels.dtw_align`` returns the path of the recursion behind ``mcd_db`` with the bits of ``dtw_cost`` in its
total, so with ``pitch`` on it replaces that launch and feeds both; ``kernels.pitch_path_accum`` adds up, over the path's
cells, how many there are, how many have both frames voiced, how many differ in voicing, how many both-voiced ones are
more than 20 % apart, and the squared F0 difference.  Pooled over the held-out set: ``f0_rmse_cents`` = sqrt(sum d^2 / both),
``gpe`` = gross / both (both None while no cell has both frames voiced - an untrained generator), ``vuv_err`` = differing /
cells, and ``voiced/fake``, ``voiced/real``, the share of voiced frames on each side.  Like ``mcd_db`` these are distances
to ONE real take of the word: two speakers of a word differ in F0 by hundreds of cents, so only the trend over training on
the fixed set says something.

What the numbers do NOT say: the held-out clips are few and fixed, so the critic numbers are a trend, not an estimate with
error bars; and a long-term average spectrum is blind to everything temporal - a sample can match it and still be
unintelligible.  It answers "is the energy in the right bands", nothing more.

Weight caches: a captured optimiser step rewrites parameters through raw pointers and bumps neither version nor epoch, so an
eager forward between two replays would find stale materialised weights (and, on bf16 storage, stale bfloat16 images).
``run`` therefore starts with ``common.bump_param_epoch`` over the parameters it is about to use and ``refresh_weights()`` on
both networks; captured graphs re-materialise inside themselves, so this costs them nothing."""
import contextlib
import json
import math

import numpy as np
import torch

from . import common
from . import kernels as K
from .extras import feature_penalty_fused

DB_FLOOR = 1e-10
_ACC_D, _ACC_G, _PEN, _LTAS, _FRAMES, _MCD, _NN, _COVER, _HIT, _DIV, _WORDS = 0, 6, 12, 13, 14, 15, 16, 17, 18, 19, 20
MCD_DB = 10.0 / math.log(10.0) * math.sqrt(2.0)          # the mel-cepstral distance's constant: natural-log cepstra -> dB
# pitch=True: further words BEHIND the others - the five sums of kernels.pitch_path_accum, the fakes' voiced frames, their frames
_PSUMS, _VOICED, _PFRAMES, _PITCH_WORDS = _WORDS, _WORDS + 5, _WORDS + 6, 7
PITCH_SR, PITCH_REF_HZ = 8000.0, 50.0                    # cents are 1200 log2(F0 / 50 Hz) at the models' 8 kHz


def power_db(p):
    """10 log10(P + 1e-10) in float64 (the logarithm is taken here, not in the kernel)"""
    return 10.0 * torch.log10(p.double() + DB_FLOOR)


def _crossed_sums(M, same):
    """M [Nf, Nr] float64, same [Nf, Nr] bool -> (sum of the row minima, sum of the column minima, number of rows whose
    minimum is attained in a column with ``same``), tensors where M lives"""
    rowmin = M.min(1).values
    hit = ((M == rowmin[:, None]) & same).any(1)
    return rowmin.sum(), M.min(0).values.sum(), hit.sum()


def crossed_scores(M, same):
    """M [Nf, Nr]: the distance of fake i to real clip j; same [Nf, Nr] bool: fake i and real clip j carry the same word
    -> dict(nn_db: mean over i of min_j M, cover_db: mean over j of min_i M, word_hit: the share of fakes i for which some j
    with same[i, j] ATTAINS the row minimum (a tie with another word's clip counts as a hit), chance: the mean over i of
    same[i].sum() / Nr - the hit rate of a uniform guess)"""
    M = torch.as_tensor(M).double()
    same = torch.as_tensor(same).to(M.device).bool()
    assert M.dim() == 2 and same.shape == M.shape and M.numel() > 0, (tuple(M.shape), tuple(same.shape))
    nf, nr = M.shape
    nn, cover, hit = _crossed_sums(M, same)
    return dict(nn_db=float(nn) / nf, cover_db=float(cover) / nr, word_hit=float(hit) / nf,
                chance=float(same.double().sum(1).div(nr).mean()))


def _pair_db(total, nf_a, nf_b):
    """raw DTW totals and the two frame counts (broadcast against each other) -> float64 dB"""
    return MCD_DB * total.double() / (nf_a + nf_b).double()


def pitch_cents(lag, peak, vthr=0.5, pfloor=1e-6):
    """lag [..] int32 and peak [.., 4] as ``kernels.pitch_frames`` (or ``audio.pitch64``) leaves them -> fp32 [..]: the frame's
    F0 in cents above 50 Hz, or -1 where it is unvoiced.  Elementwise torch where the inputs live, in float64, stored as
    fp32 (the logarithm and the refinement are taken here, not in the kernel).  Voiced: lag > 0, phi(lag) >= ``vthr`` and the
    window's mean power e0 / 256 >= ``pfloor``.  The lag is refined by the parabola through phi(lag - 1), phi(lag),
    phi(lag + 1): with den = phi- - 2 phi0 + phi+, delta = 0.5 (phi- - phi+) / den clamped to [-0.5, 0.5] when den < 0, else
    0; cents = 1200 log2((8000 / (lag + delta)) / 50).  Every voiced value is above 380, so a negative value is the flag."""
    lag = torch.as_tensor(lag)
    p = torch.as_tensor(peak).to(lag.device).double()
    pm, p0, pp, power = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    voiced = (lag > 0) & (p0 >= vthr) & (power >= pfloor)
    den = pm - 2.0 * p0 + pp
    curved = den < 0
    delta = torch.where(curved, (0.5 * (pm - pp) / torch.where(curved, den, torch.ones_like(den))).clamp(-0.5, 0.5),
                        torch.zeros_like(den))
    period = torch.where(voiced, lag.double() + delta, torch.ones_like(den))
    cents = 1200.0 * torch.log2((PITCH_SR / period) / PITCH_REF_HZ)
    return torch.where(voiced, cents, torch.full_like(cents, -1.0)).float()


def pitch_path_sums64(pc_a, pc_b, lo, hi, nf_b=None, gross=None):
    """the rule of ``kernels.pitch_path_accum`` in float64 numpy: pc_a [B, Fa], pc_b [B, Fb] cents (negative: unvoiced), lo /
    hi [B, Fb] and nf_b [B] (None: Fb; clamped to [1, Fb]) -> float64 [B, 5]: over the cells (column j < nf_b[b], rows
    lo[j]..hi[j], row indices clamped into [0, Fa - 1]) their number, those with both frames voiced, those whose voicing
    differs, the both-voiced ones with |a - b| > gross, and the sum of (a - b)^2 over the both-voiced ones.  ``gross`` is
    taken at its fp32 value (default: that of 1200 log2(1.2)).  Columns at or past the count are never read."""
    tn = lambda v: v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)          # noqa: E731
    pc_a, pc_b, lo, hi = tn(pc_a), tn(pc_b), tn(lo), tn(hi)
    gross = float(np.float32(K.PITCH_GROSS if gross is None else gross))
    B, Fa, Fb = pc_a.shape[0], pc_a.shape[1], pc_b.shape[1]
    out = np.zeros((B, 5))
    for b in range(B):
        m = Fb if nf_b is None else max(1, min(int(tn(nf_b)[b]), Fb))
        for j in range(m):
            r0, r1 = (max(0, min(int(v), Fa - 1)) for v in (lo[b, j], hi[b, j]))
            a, vb = pc_a[b, r0:r1 + 1].astype(np.float64), float(pc_b[b, j])
            both = (a >= 0) & (vb >= 0)
            d = a[both] - vb
            out[b] += (len(a), both.sum(), ((a >= 0) != (vb >= 0)).sum(), (np.abs(d) > gross).sum(), (d * d).sum())
    return out


def pitch_scores(sums):
    """[B, 5] sums of ``kernels.pitch_path_accum`` (tensor or array) -> dict of [B] float64 tensors: f0_rmse_cents = sqrt(sum d^2
    / both) and gpe = gross / both (NaN where no cell has both frames voiced), vuv_err = differing / cells, cells"""
    s = torch.as_tensor(sums).double()
    cells, both, differ, far, ss = s.unbind(-1)
    nan = torch.full_like(ss, float('nan'))
    some = both > 0
    safe = torch.where(some, both, torch.ones_like(both))
    return dict(f0_rmse_cents=torch.where(some, (ss / safe).sqrt(), nan), vuv_err=differ / cells,
                gpe=torch.where(some, far / safe, nan), cells=cells)


def finish_scores(a):
    """the host's half of ``kernels.score_accum``: six words -> (loss, accuracy, mean, std)"""
    a0, a1, a2, a3, a4, a5 = (float(v) for v in a)
    mean = a4 / a2
    return a1 / a0, a3 / a2, mean, math.sqrt(max(0.0, a5 / a2 - mean * mean))


class Evaluator(object):
    def __init__(self, g, d, e_g, e_d, heldout, batch_size, maxlen, device, batches=4, seed=0, ema=None, on_eval=None,
                 path=None, aligned=False, crossed=False, draws=1, pitch=False):
        """``heldout``: the validation loader ``dataset.dataloader`` returns (``next()`` -> [epoch, batch, samples, lengths,
        keys, cseq, clen]) or a list of such minibatches; ``batches`` of them are taken NOW (see the module text: build the
        evaluator before the training loader's first ``next()`` when this is a loader).  ``ema``: an ``optim.EMA`` - the pass
        runs inside ``ema.applied()``, as samples do.  ``on_eval(result)``: receives every result dict; ``path``: every
        result is appended there as one JSON line with ``kind: 'E'``.  ``aligned``: also measure ``mcd_db``, the
        mel-cepstral distance of every fake along its time-warping path to the real clip of the same word (module text)
        - the real clips' cepstra are computed now and kept.  ``crossed`` / ``draws`` (both need ``aligned``): also measure
        ``nn_db``, ``cover_db``, ``word_hit`` and ``word_hit/chance`` / ``div_db`` and ``real_div_db`` (module text).
        ``pitch`` (needs ``aligned``): also measure ``f0_rmse_cents``, ``vuv_err``, ``gpe``, ``voiced/fake`` and
        ``voiced/real`` along the time-warping path (module text) - the real clips' cents are computed now and kept."""
        self.g, self.d, self.e_g, self.e_d = g, d, e_g, e_d
        self.B, self.maxlen, self.dev = int(batch_size), maxlen, torch.device(device)
        self.ema, self.on_eval, self.path = ema, on_eval, path
        fs = g._frame_size
        self.nframes = (maxlen + fs - 1) // fs
        self.L = self.nframes * fs
        self.aligned, self.crossed, self.draws, self.pitch = bool(aligned), bool(crossed), int(draws), bool(pitch)
        if self.draws < 1 or self.draws != draws:
            raise ValueError('Evaluator(draws=%r): a whole number of draws per word, 1 or more' % (draws,))
        if (self.crossed or self.draws > 1) and not self.aligned:
            raise ValueError('Evaluator(crossed=%r, draws=%r) compares cepstra: it needs aligned=True' % (crossed, draws))
        if self.pitch and not self.aligned:
            raise ValueError('Evaluator(pitch=%r) compares F0 along the cepstra\'s path: it needs aligned=True' % (pitch,))
        if self.aligned and K.lt_frames(self.L) > K.DTW_MAX_FRAMES:
            raise ValueError('Evaluator(aligned=True): clips of %d samples have %d frames; kernels.dtw_cost takes at most %d'
                             % (self.L, K.lt_frames(self.L), K.DTW_MAX_FRAMES))
        took = list(heldout[:batches]) if isinstance(heldout, (list, tuple)) else [next(heldout) for _ in range(batches)]
        assert len(took) == batches >= 1, (len(took), batches)
        rng = torch.Generator(device=self.dev).manual_seed(int(seed))      # private: no training stream moves
        self.set = []
        for mb in took:
            _, _, samples, lengths, _, cseq, clen = mb
            x = np.zeros((self.B, self.L), dtype=np.float32)
            n = min(self.L, samples.shape[1])
            x[:, :n] = samples[:, :n]
            real, real_len = self._up(x, torch.float32), self._up(lengths, torch.long)
            z = torch.randn(self.B, self.nframes, g._noise_size, device=self.dev, generator=rng)
            u = torch.rand(self.nframes, self.B, device=self.dev, generator=rng)
            power = K.ltas_power(real, real_len)
            self.set.append(dict(real=real, real_len=real_len, cs=self._up(cseq, torch.long), cl=self._up(clen, torch.long),
                                 z=z, u=u, real_power=power, real_db=power_db(power)))
            if self.aligned:
                nf = torch.empty(self.B, dtype=torch.int32, device=self.dev)
                self.set[-1].update(real_cep=K.melcep_frames(real, real_len, nframes=nf), real_nf=nf)
            if self.pitch:
                self.set[-1].update(real_cents=pitch_cents(*K.pitch_frames(real, real_len)))
        self.clips = self.B * batches
        self._chance = self.real_div_db = None
        if self.crossed or self.draws > 1:
            words = [[tuple(np.asarray(mb[5])[b, :int(np.asarray(mb[6])[b])].tolist()) for b in range(self.B)] for mb in took]
        if self.crossed:
            for mb, w in zip(self.set, words):
                same = np.array([[a == b for b in w] for a in w], dtype=bool)
                mb['same'] = self._up(same, torch.bool)
            self._chance = float(np.mean([sum(a == b for b in w) / float(self.B) for w in words for a in w]))
        if self.draws > 1:
            for mb in self.set:          # after every first draw: those keep the bits of an evaluator with draws=1
                mb['more'] = [(torch.randn(self.B, self.nframes, g._noise_size, device=self.dev, generator=rng),
                               torch.rand(self.nframes, self.B, device=self.dev, generator=rng)) for _ in range(self.draws - 1)]
            # draw pairs (p < q) of every clip, as rows of the bank of draws * B fakes a pass fills
            pq = [(p * self.B + b, q * self.B + b) for p in range(self.draws) for q in range(p + 1, self.draws)
                  for b in range(self.B)]
            self._pairs = tuple(self._up(np.array(c, dtype=np.int32), torch.int32) for c in zip(*pq))
            # the yardstick: all pairs i < j of held-out real clips that share a word, one launch over the concatenated cepstra
            flat = [w for ws in words for w in ws]
            ij = [(i, j) for i in range(len(flat)) for j in range(i + 1, len(flat)) if flat[i] == flat[j]]
            if ij:
                cep = torch.cat([mb['real_cep'] for mb in self.set])
                nf = torch.cat([mb['real_nf'] for mb in self.set])
                ia, ib = (self._up(np.array(c, dtype=np.int32), torch.int32) for c in zip(*ij))
                tot = K.dtw_pairs(cep, nf, cep, nf, ia, ib)
                self.real_div_db = float(_pair_db(tot, nf[ia.long()], nf[ib.long()]).mean())
        self._buf = torch.zeros(_WORDS + (_PITCH_WORDS if self.pitch else 0), dtype=torch.float64, device=self.dev)
        self.voiced_real = None
        if self.pitch:
            F = K.lt_frames(self.L)
            self._frame = torch.arange(F, device=self.dev)
            # the decisions of dtw_align, for the widest fake a pass can meet: allocated once
            self._align_ws = torch.empty(max(self.B * K.dtw_align_ws(F, F), 4) // 4, dtype=torch.int32, device=self.dev)
            on = sum(int(((mb['real_cents'] >= 0) & (self._frame[None, :] < mb['real_nf'][:, None])).sum()) for mb in self.set)
            self.voiced_real = on / float(sum(int(mb['real_nf'].sum()) for mb in self.set))

    def _up(self, a, dtype):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(dtype).to(self.dev)

    def run(self, gen_iter=None, dis_iter=None, parts=False):
        """one pass over the fixed held-out set -> dict(loss_d, acc_d, cls_d/mean, cls_d/std, loss_g, acc_g, cls_g/mean,
        cls_g/std, feature_penalty, ltas_db, frames/mean, clips, gen_iter, dis_iter; with ``aligned`` also mcd_db, with
        ``crossed`` nn_db, cover_db, word_hit and word_hit/chance, with ``draws`` of 2 or more div_db and real_div_db).
        ``parts=True``: returns (dict, list) with, per minibatch, the waves, lengths, logits, conv activations and powers the
        numbers were computed from (with ``aligned`` also cep, nf, real_cep, real_nf and dtw, the raw totals; with
        ``crossed`` cross, the raw [B, B] totals fake x real, and same; with ``draws`` bank_cep [draws * B, F, 16] and bank_nf,
        the cepstra and counts of every draw (draw p of clip b in row p * B + b), and pair_ia, pair_ib, pair_dtw: the rows
        compared and their raw totals)."""
        g, d, e_g, e_d = self.g, self.d, self.e_g, self.e_d
        fs = g._frame_size
        buf, kept = self._buf, []
        averaged = self.ema.applied() if self.ema is not None else contextlib.nullcontext()
        with torch.no_grad(), averaged:
            # (inside ``applied()`` the parameters of g and e_g hold the averages and their epochs are already bumped)
            stale = list(d.parameters()) + list(e_d.parameters())
            if self.ema is None:
                stale += list(g.parameters()) + list(e_g.parameters())
            common.bump_param_epoch(stale)
            g.refresh_weights()
            d.refresh_weights()
            buf.zero_()
            for mb in self.set:
                embed_d, embed_g = e_d(mb['cs'], mb['cl']), e_g(mb['cs'], mb['cl'])
                cls_d, hs_d, hl_d, nf_d = d(mb['real'], mb['real_len'], embed_d)
                nf_d = nf_d.contiguous()
                K.score_accum(cls_d, nf_d, 0.9, True, buf[_ACC_D:_ACC_D + 6])
                fake, _, _, fake_len = g.generate(embed_g, z=mb['z'], u=mb['u'])
                cls_g, hs_g, hl_g, nf_g = d(fake, fake_len, embed_d)
                nf_g = nf_g.contiguous()
                K.score_accum(cls_g, nf_g, 0.0, False, buf[_ACC_G:_ACC_G + 6])
                pen = feature_penalty_fused(hs_d, hl_d, hs_g, hl_g, self.B)
                power = K.ltas_power(fake, fake_len)
                dist = (power_db(power) - mb['real_db']).pow(2).mean(1).sqrt()
                buf[_PEN] += pen.double()
                buf[_LTAS] += dist.sum()
                buf[_FRAMES] += (fake_len // fs).sum()
                if parts:
                    kept.append(dict(wave=fake, length=fake_len, cls_d=cls_d, cls_g=cls_g, nf_d=nf_d, nf_g=nf_g, hs_d=hs_d,
                                     hl_d=hl_d, hs_g=hs_g, hl_g=hl_g, power=power, real_power=mb['real_power']))
                if self.aligned:
                    nf = torch.empty(self.B, dtype=torch.int32, device=self.dev)
                    cep = K.melcep_frames(fake, fake_len, nframes=nf)
                    if self.pitch:
                        # the total has dtw_cost's bits (the same recursion), so one launch feeds mcd_db and the path
                        dtw, lo, hi = K.dtw_align(cep, nf, mb['real_cep'], mb['real_nf'], workspace=self._align_ws)
                    else:
                        dtw = K.dtw_cost(cep, nf, mb['real_cep'], mb['real_nf'])
                    buf[_MCD] += (dtw.double() / (nf + mb['real_nf']).double()).sum()
                    if parts:
                        kept[-1].update(cep=cep, nf=nf, real_cep=mb['real_cep'], real_nf=mb['real_nf'], dtw=dtw)
                if self.pitch:
                    lag, peak = K.pitch_frames(fake, fake_len)
                    cents = pitch_cents(lag, peak)
                    sums = K.pitch_path_accum(cents, mb['real_cents'], lo, hi, mb['real_nf'])
                    buf[_PSUMS:_PSUMS + 5] += sums.double().sum(0)
                    buf[_VOICED] += ((cents >= 0) & (self._frame[None, :cents.size(1)] < nf[:, None])).sum()
                    buf[_PFRAMES] += nf.sum()
                    if parts:
                        kept[-1].update(lag=lag, peak=peak, cents=cents, real_cents=mb['real_cents'], lo=lo, hi=hi,
                                        pitch_sums=sums)
                if self.crossed:
                    cross = K.dtw_pairs(cep, nf, mb['real_cep'], mb['real_nf'])
                    nn, cover, hit = _crossed_sums(_pair_db(cross, nf[:, None], mb['real_nf'][None, :]), mb['same'])
                    buf[_NN] += nn
                    buf[_COVER] += cover
                    buf[_HIT] += hit
                    if parts:
                        kept[-1].update(cross=cross, same=mb['same'])
                if self.draws > 1:
                    # the extra fakes: no critic pass; every draw's cepstra go into one bank at the widest draw's capacity
                    # (rows past a clip's count are never read, so what the bank holds there does not matter)
                    ceps, nfs = [cep], torch.empty(self.draws * self.B, dtype=torch.int32, device=self.dev)
                    nfs[:self.B] = nf
                    for q, (z, u) in enumerate(mb['more'], 1):
                        more, _, _, more_len = g.generate(embed_g, z=z, u=u)
                        ceps.append(K.melcep_frames(more, more_len, nframes=nfs[q * self.B:(q + 1) * self.B]))
                    bank = torch.zeros(self.draws * self.B, max(c.size(1) for c in ceps), K.CEP_WIDTH, device=self.dev)
                    for q, c in enumerate(ceps):
                        bank[q * self.B:(q + 1) * self.B, :c.size(1)] = c
                    ia, ib = self._pairs
                    tot = K.dtw_pairs(bank, nfs, bank, nfs, ia, ib)
                    buf[_DIV] += _pair_db(tot, nfs[ia.long()], nfs[ib.long()]).sum()
                    if parts:
                        kept[-1].update(bank_cep=bank, bank_nf=nfs, pair_ia=ia, pair_ib=ib, pair_dtw=tot)
            host = buf.cpu().tolist()          # the pass's ONE copy to the host
        res = {}
        for tag, o in (('d', _ACC_D), ('g', _ACC_G)):
            loss, acc, mean, std = finish_scores(host[o:o + 6])
            res['loss_' + tag], res['acc_' + tag], res['cls_%s/mean' % tag], res['cls_%s/std' % tag] = loss, acc, mean, std
        res['feature_penalty'] = host[_PEN] / len(self.set)
        res['ltas_db'] = host[_LTAS] / self.clips
        res['frames/mean'] = host[_FRAMES] / self.clips
        if self.aligned:
            res['mcd_db'] = MCD_DB * host[_MCD] / self.clips
        if self.pitch:
            cells, both, differ, far, ss = host[_PSUMS:_PSUMS + 5]
            res['f0_rmse_cents'] = math.sqrt(ss / both) if both > 0 else None
            res['vuv_err'] = differ / cells
            res['gpe'] = far / both if both > 0 else None
            res['voiced/fake'], res['voiced/real'] = host[_VOICED] / host[_PFRAMES], self.voiced_real
        if self.crossed:
            res['nn_db'], res['cover_db'] = host[_NN] / self.clips, host[_COVER] / self.clips
            res['word_hit'], res['word_hit/chance'] = host[_HIT] / self.clips, self._chance
        if self.draws > 1:
            res['div_db'] = host[_DIV] / (self.clips * (self.draws * (self.draws - 1) // 2))
            res['real_div_db'] = self.real_div_db
        res['clips'] = self.clips
        res['gen_iter'] = None if gen_iter is None else int(gen_iter)
        res['dis_iter'] = None if dis_iter is None else int(dis_iter)
        if self.on_eval is not None:
            self.on_eval(res)
        if self.path is not None:
            with open(self.path, 'a') as f:
                f.write(json.dumps(dict(kind='E', **res)) + '\n')
        return (res, kept) if parts else res


def aligned_distance(wave_a, len_a, wave_b, len_b):
    """wave_a [B, La], wave_b [B, Lb] fp32 device clips (unit stride along time) with their int64 lengths (or None: whole
    rows) -> [B] float64: per pair the mel-cepstral distance in dB along the time-warping path, what ``Evaluator(aligned=
    True)`` averages into ``mcd_db`` (module text).  0 for a clip against itself; at most 1024 frames (131200 samples) a
    side."""
    for w in (wave_a, wave_b):
        if K.lt_frames(w.size(1)) > K.DTW_MAX_FRAMES:
            raise ValueError('aligned_distance: clips of %d samples have more than %d frames' % (w.size(1), K.DTW_MAX_FRAMES))
    B = wave_a.size(0)
    nf_a = torch.empty(B, dtype=torch.int32, device=wave_a.device)
    nf_b = torch.empty(B, dtype=torch.int32, device=wave_a.device)
    cep_a = K.melcep_frames(wave_a, len_a, nframes=nf_a)
    cep_b = K.melcep_frames(wave_b, len_b, nframes=nf_b)
    return MCD_DB * K.dtw_cost(cep_a, nf_a, cep_b, nf_b).double() / (nf_a + nf_b).double()


def pitch_distance(wave_a, len_a, wave_b, len_b, vthr=0.5, pfloor=1e-6):
    """wave_a [B, La], wave_b [B, Lb] with their lengths as ``aligned_distance`` takes them -> dict of [B] float64 tensors, per
    pair along the time-warping path of their cepstra (a's frames the rows): ``f0_rmse_cents`` (the root mean square F0
    difference over the cells with both frames voiced; NaN where there is none), ``vuv_err`` (the share of cells whose
    voicing differs), ``gpe`` (the share of both-voiced cells more than 20 % apart; NaN as above) and ``cells``.  What
    ``Evaluator(aligned=True, pitch=True)`` pools over the held-out set (module text); two ``melcep_frames``, two
    ``pitch_frames``, one ``dtw_align`` and one ``pitch_path_accum`` launch."""
    for w in (wave_a, wave_b):
        if K.lt_frames(w.size(1)) > K.DTW_MAX_FRAMES:
            raise ValueError('pitch_distance: clips of %d samples have more than %d frames' % (w.size(1), K.DTW_MAX_FRAMES))
    B = wave_a.size(0)
    nf_a = torch.empty(B, dtype=torch.int32, device=wave_a.device)
    nf_b = torch.empty(B, dtype=torch.int32, device=wave_a.device)
    cep_a = K.melcep_frames(wave_a, len_a, nframes=nf_a)
    cep_b = K.melcep_frames(wave_b, len_b, nframes=nf_b)
    _, lo, hi = K.dtw_align(cep_a, nf_a, cep_b, nf_b)
    pc_a = pitch_cents(*K.pitch_frames(wave_a, len_a), vthr=vthr, pfloor=pfloor)
    pc_b = pitch_cents(*K.pitch_frames(wave_b, len_b), vthr=vthr, pfloor=pfloor)
    return pitch_scores(K.pitch_path_accum(pc_a, pc_b, lo, hi, nf_b))


def aligned_distance_matrix(wave_a, len_a, wave_b, len_b):
    """wave_a [Na, La], wave_b [Nb, Lb] as ``aligned_distance`` takes them -> [Na, Nb] float64: ``aligned_distance`` of every
    clip of a against every clip of b, MCD_DB total / (n_i + m_j) - two ``melcep_frames`` launches and one ``dtw_pairs``
    launch, with the bits ``aligned_distance`` gives pair by pair.  At most 1024 frames (131200 samples) a side."""
    for w in (wave_a, wave_b):
        if K.lt_frames(w.size(1)) > K.DTW_MAX_FRAMES:
            raise ValueError('aligned_distance_matrix: clips of %d samples have more than %d frames'
                             % (w.size(1), K.DTW_MAX_FRAMES))
    nf_a = torch.empty(wave_a.size(0), dtype=torch.int32, device=wave_a.device)
    nf_b = torch.empty(wave_b.size(0), dtype=torch.int32, device=wave_a.device)
    cep_a = K.melcep_frames(wave_a, len_a, nframes=nf_a)
    cep_b = K.melcep_frames(wave_b, len_b, nframes=nf_b)
    return _pair_db(K.dtw_pairs(cep_a, nf_a, cep_b, nf_b), nf_a[:, None], nf_b[None, :])
