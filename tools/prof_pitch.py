"""What do the two kernels of the pitch measures cost, next to the stock device forms, and what does the option add to a pass?

  * ``kernels.pitch_frames`` at (B 64, L 8192) and (B 32, L 40000) against the stock form (``unfold`` to segments, centring,
    one batched ``matmul`` of the window against its lagged copies, energies by ``cumsum``, the first-strong-peak logic with
    ``argmax``), alternating in the same run; device events around ``--launches`` back-to-back launches, medians of
    ``--rounds`` rounds;
  * ``kernels.pitch_path_accum`` at 63 and 311 frames a side on the paths ``kernels.dtw_align`` returns, against a masked torch
    reduction over a [B, Fa, Fb] mask, the same way;
  * one ``evaluate.Evaluator.run()`` at the C2 widths (the setup of tools/prof_eval.py) with ``aligned`` alone and with
    ``pitch``, alternating.  ``dtw_cost`` and ``dtw_align`` are timed beside the path sums at the two kernel shapes; the
    first of them, B 64 at 63 frames a side, is the shape of a held-out minibatch of that pass (8192-sample clips).

    python tools/prof_pitch.py [--out profiles/eval_pitch.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.prof_eval import med, setup, timed          # noqa: E402


def work_pitch_frames(B, L):
    """-> (flops, bytes) of one pitch_frames launch without nccf: five fmaf chains of 256 terms per (frame, lane) of the 64
    lanes that own the lags; the clip read once, lag and peak written once"""
    F = (L - 256) // 128 + 1 if L >= 256 else 1
    return 2.0 * 5 * 256 * 64 * B * F, 4.0 * (B * L + B * F * 5)


def stock_pitch(x, octf=0.9):
    """whole rows only (no lengths): -> (lag [B, F], phi [B, F, 110])"""
    B, L = x.shape
    F = (L - 256) // 128 + 1
    xp = torch.nn.functional.pad(x, (0, (F - 1) * 128 + 384 - L))
    valid = (torch.arange(F, device=x.device)[:, None] * 128 + torch.arange(384, device=x.device)[None, :]) < L
    seg = xp.unfold(1, 384, 128)                                              # [B, F, 384]
    mean = seg.sum(-1, keepdim=True) / valid.sum(-1)[None, :, None]
    seg = torch.where(valid[None], seg - mean, torch.zeros_like(seg))
    head = seg[..., :256]
    lagged = seg.unfold(2, 256, 1)[:, :, 19:129]                              # [B, F, 110, 256] (a view)
    r = torch.matmul(lagged, head.unsqueeze(-1)).squeeze(-1)
    cs = torch.nn.functional.pad((seg * seg).cumsum(-1), (1, 0))
    e = cs[..., 19 + 256:129 + 256] - cs[..., 19:129]
    den = cs[..., 256:257] * e
    phi = torch.where(den > 0, r / den.clamp_min(1e-38).sqrt(), torch.zeros_like(r))
    mid = phi[..., 1:-1]
    M = mid.max(-1, keepdim=True).values
    ok = (mid >= phi[..., :-2]) & (mid >= phi[..., 2:]) & (mid >= octf * M) & (M > 0)
    lag = torch.where(ok.any(-1), ok.int().argmax(-1) + 20, torch.zeros_like(M[..., 0], dtype=torch.long))
    return lag, phi


def stock_path_sums(pc_a, pc_b, lo, hi, nf_b, gross):
    B, Fa, Fb = pc_a.size(0), pc_a.size(1), pc_b.size(1)
    i = torch.arange(Fa, device=pc_a.device)[None, :, None]
    j = torch.arange(Fb, device=pc_a.device)[None, None, :]
    on = (i >= lo[:, None, :]) & (i <= hi[:, None, :]) & (j < nf_b[:, None, None])
    va, vb = pc_a[:, :, None] >= 0, pc_b[:, None, :] >= 0
    both = on & va & vb
    d = torch.where(both, pc_a[:, :, None] - pc_b[:, None, :], torch.zeros((), device=pc_a.device))
    return torch.stack([on.sum((1, 2)).float(), both.sum((1, 2)).float(), (on & (va != vb)).sum((1, 2)).float(),
                        (d.abs() > gross).sum((1, 2)).float(), (d * d).sum((1, 2))], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--batches', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from audiogan_amd import evaluate
    from audiogan_amd import kernels as K
    dev = torch.device('cuda')
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    gen = torch.Generator().manual_seed(1)
    say('pitch measures: us per launch, device events around %d back-to-back launches, rounds in the order they were taken'
        % args.launches)
    for B, L in ((64, 8192), (32, 40000)):
        t_ = torch.arange(L)[None, :] / 8000.0
        f0 = 80.0 + 300.0 * torch.rand(B, 1, generator=gen)
        x = sum(torch.sin(2 * torch.pi * k * f0 * t_) / k for k in range(1, 9)) * 0.2 + 0.05 * torch.randn(B, L, generator=gen)
        x = x.to(dev)
        F = K.lt_frames(L)
        lag = torch.empty(B, F, dtype=torch.int32, device=dev)
        peak = torch.empty(B, F, 4, device=dev)
        nccf = torch.empty(B, F, K.PITCH_NCCF, device=dev)
        K.pitch_frames(x, None, lag=lag, peak=peak, nccf=nccf)
        name = K.lib.ag_last_kernel().decode()
        slag, sphi = stock_pitch(x)
        say('B %d, L %d (%d frames per clip), %s; against the stock form: largest |phi| difference %.1e, lags equal in %.2f %% '
            'of the frames' % (B, L, F, name, float((nccf[..., :K.PITCH_LAGS] - sphi).abs().max()),
                               100.0 * float((lag.long() == slag).float().mean())))
        flops, nbytes = work_pitch_frames(B, L)
        t = dict(k=[], kn=[], st=[])
        for r in range(args.rounds):
            t['k'].append(timed(lambda: K.pitch_frames(x, None, lag=lag, peak=peak), 10, args.launches) * 1e3)
            t['kn'].append(timed(lambda: K.pitch_frames(x, None, lag=lag, peak=peak, nccf=nccf), 10, args.launches) * 1e3)
            t['st'].append(timed(lambda: stock_pitch(x), 3, max(1, args.launches // 10)) * 1e3)
            say('round %d  pitch_frames %9.2f   with nccf %9.2f   unfold + matmul + cumsum + argmax %9.2f'
                % (r + 1, t['k'][-1], t['kn'][-1], t['st'][-1]))
        say('median: pitch_frames %.2f us (%.2f TFLOP/s of the issued chains, %.1f GB/s of its inputs and outputs), with nccf '
            '%.2f us;  stock form %.2f us;  library / stock = %.3f'
            % (med(t['k']), flops / med(t['k']) / 1e6, nbytes / med(t['k']) / 1e3, med(t['kn']), med(t['st']),
               med(t['k']) / med(t['st'])))
        # the path sums at this frame count, on the paths of dtw_align between the clips and their flipped batch
        nf = torch.empty(B, dtype=torch.int32, device=dev)
        cep = K.melcep_frames(x, None, nframes=nf)
        cb = cep.flip(0).contiguous()
        ws = torch.empty(max(B * K.dtw_align_ws(F, F), 4) // 4, dtype=torch.int32, device=dev)
        total, lo, hi = K.dtw_align(cep, nf, cb, nf, workspace=ws)
        cents = evaluate.pitch_cents(lag, peak)
        cents_b = cents.flip(0).contiguous()
        out = torch.empty(B, K.PITCH_PATH_WORDS, device=dev)
        K.pitch_path_accum(cents, cents_b, lo, hi, nf, out=out)
        ref = stock_path_sums(cents, cents_b, lo, hi, nf, K.PITCH_GROSS)
        same = bool((out[:, :4] == ref[:, :4]).all())
        rel = float(((out[:, 4] - ref[:, 4]).abs() / ref[:, 4].clamp_min(1e-30)).max())
        tp = dict(k=[], st=[], cost=[], align=[])
        dtw = torch.empty(B, device=dev)
        for r in range(args.rounds):
            tp['k'].append(timed(lambda: K.pitch_path_accum(cents, cents_b, lo, hi, nf, out=out), 10, args.launches) * 1e3)
            tp['st'].append(timed(lambda: stock_path_sums(cents, cents_b, lo, hi, nf, K.PITCH_GROSS), 3,
                                  max(1, args.launches // 10)) * 1e3)
            tp['cost'].append(timed(lambda: K.dtw_cost(cep, nf, cb, nf, out=dtw), 10, args.launches) * 1e3)
            tp['align'].append(timed(lambda: K.dtw_align(cep, nf, cb, nf, total=total, lo=lo, hi=hi, workspace=ws), 10,
                                     args.launches) * 1e3)
            say('round %d  pitch_path_accum (%d x %d frames) %9.2f   masked torch reduction %9.2f   dtw_cost %9.2f   dtw_align %9.2f'
                % (r + 1, F, F, tp['k'][-1], tp['st'][-1], tp['cost'][-1], tp['align'][-1]))
        say('median: pitch_path_accum %.2f us;  masked reduction over [B, Fa, Fb] %.2f us;  library / stock = %.3f (counts equal: '
            '%s, sum d^2 within %.1e);  dtw_align %.2f us / dtw_cost %.2f us = %.2f'
            % (med(tp['k']), med(tp['st']), med(tp['k']) / med(tp['st']), same, rel, med(tp['align']), med(tp['cost']),
               med(tp['align']) / med(tp['cost'])))

    ev, lp = setup(args.batch, args.batches, dev)
    heldout = [(0, 0, mb['real'].cpu().numpy(), mb['real_len'].cpu().numpy(), None, mb['cs'].cpu().numpy(),
                mb['cl'].cpu().numpy()) for mb in ev.set]
    mk = lambda **kw: evaluate.Evaluator(ev.g, ev.d, ev.e_g, ev.e_d, heldout, ev.B, ev.maxlen, dev, batches=args.batches,          # noqa: E731
                                         seed=0, aligned=True, **kw)
    ev_a, ev_p = mk(), mk(pitch=True)
    for e in (ev_a, ev_p):          # full-length fakes, the long end for the new kernels
        for mb in e.set:
            mb['u'].fill_(1.0)
    res = ev_p.run()
    say('Evaluator.run() at the C2 widths, %d clips per minibatch, %d held-out minibatches, full-length fakes (%.1f frames of '
        '%d: %d samples, %d cepstral frames a side - the first shape above); ms per pass, device events around %d passes ending '
        'in a synchronise;  untrained: f0_rmse_cents %r, vuv_err %.3f, voiced/fake %.3f, voiced/real %.3f'
        % (args.batch, args.batches, res['frames/mean'], ev.nframes, ev.L, K.lt_frames(ev.L), args.passes,
           res['f0_rmse_cents'], res['vuv_err'], res['voiced/fake'], res['voiced/real']))
    t_a, t_p = [], []
    for r in range(args.rounds):
        t_a.append(timed(ev_a.run, 1, args.passes))
        t_p.append(timed(ev_p.run, 1, args.passes))
        say('round %d  aligned alone %9.2f   with pitch %9.2f' % (r + 1, t_a[-1], t_p[-1]))
    say('median: aligned alone %.2f ms, with pitch %.2f ms: +%.2f ms per pass (+%.3f per held-out minibatch)'
        % (med(t_a), med(t_p), med(t_p) - med(t_a), (med(t_p) - med(t_a)) / args.batches))
    K.check_persist_status(dev)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
