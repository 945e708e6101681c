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
_ACC_D, _ACC_G, _PEN, _LTAS, _FRAMES, _MCD, _WORDS = 0, 6, 12, 13, 14, 15, 16
MCD_DB = 10.0 / math.log(10.0) * math.sqrt(2.0)          # the mel-cepstral distance's constant: natural-log cepstra -> dB


def power_db(p):
    """10 log10(P + 1e-10) in float64 (the logarithm is taken here, not in the kernel)"""
    return 10.0 * torch.log10(p.double() + DB_FLOOR)


def finish_scores(a):
    """the host's half of ``kernels.score_accum``: six words -> (loss, accuracy, mean, std)"""
    a0, a1, a2, a3, a4, a5 = (float(v) for v in a)
    mean = a4 / a2
    return a1 / a0, a3 / a2, mean, math.sqrt(max(0.0, a5 / a2 - mean * mean))


class Evaluator(object):
    def __init__(self, g, d, e_g, e_d, heldout, batch_size, maxlen, device, batches=4, seed=0, ema=None, on_eval=None,
                 path=None, aligned=False):
        """``heldout``: the validation loader ``dataset.dataloader`` returns (``next()`` -> [epoch, batch, samples, lengths,
        keys, cseq, clen]) or a list of such minibatches; ``batches`` of them are taken NOW (see the module text: build the
        evaluator before the training loader's first ``next()`` when this is a loader).  ``ema``: an ``optim.EMA`` - the pass
        runs inside ``ema.applied()``, as samples do.  ``on_eval(result)``: receives every result dict; ``path``: every
        result is appended there as one JSON line with ``kind: 'E'``.  ``aligned``: also measure ``mcd_db``, the
        mel-cepstral distance of every fake along its time-warping path to the real clip of the same word (module text)
        - the real clips' cepstra are computed now and kept."""
        self.g, self.d, self.e_g, self.e_d = g, d, e_g, e_d
        self.B, self.maxlen, self.dev = int(batch_size), maxlen, torch.device(device)
        self.ema, self.on_eval, self.path = ema, on_eval, path
        fs = g._frame_size
        self.nframes = (maxlen + fs - 1) // fs
        self.L = self.nframes * fs
        self.aligned = bool(aligned)
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
        self.clips = self.B * batches
        self._buf = torch.zeros(_WORDS, dtype=torch.float64, device=self.dev)

    def _up(self, a, dtype):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(dtype).to(self.dev)

    def run(self, gen_iter=None, dis_iter=None, parts=False):
        """one pass over the fixed held-out set -> dict(loss_d, acc_d, cls_d/mean, cls_d/std, loss_g, acc_g, cls_g/mean,
        cls_g/std, feature_penalty, ltas_db, frames/mean, clips, gen_iter, dis_iter; with ``aligned`` also mcd_db).
        ``parts=True``: returns (dict, list) with, per minibatch, the waves, lengths, logits, conv activations and powers the
        numbers were computed from (with ``aligned`` also cep, nf, real_cep, real_nf and dtw, the raw totals)."""
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
                    dtw = K.dtw_cost(cep, nf, mb['real_cep'], mb['real_nf'])
                    buf[_MCD] += (dtw.double() / (nf + mb['real_nf']).double()).sum()
                    if parts:
                        kept[-1].update(cep=cep, nf=nf, real_cep=mb['real_cep'], real_nf=mb['real_nf'], dtw=dtw)
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
