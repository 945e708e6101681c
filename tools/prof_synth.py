"""What does joining generated words into sentences cost, with the two launches (ag_join_facts, ag_join_clips) and with the
stock form, and how fast does ``synth.Voice.say`` talk?

  * at 1 sentence x 12 words x 8192 samples and at 16 sentences x 12 words x 16000 samples (random lengths between half a row
    and a whole one, a fade of 40 samples, pauses of 960):
      the launches    ``kernels.join_facts`` then ``kernels.join_clips``, each alone and the pair; nothing is read to the host
      the stock form  the lengths read to the host (``n.cpu()``), one masked ``abs().amax`` for the peaks, ``out.zero_()`` and
                      one ``out[s, a:b] += x * w`` per word
    device events around ``--launches`` back-to-back calls, the forms alternating, medians of ``--rounds`` rounds; microseconds,
    and for ag_join_clips GB/s of samples read plus the whole of ``out`` written.  The two forms' outputs are compared first.
  * ``Voice.say`` end to end at the C2 widths (frame 256, state 1024; untrained, so the stop draws end words at random): host
    clock around ``--says`` sentences of 12 words ending in a synchronise, seconds of audio per second.

    python tools/prof_synth.py [--out profiles/synth_join.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.prof_eval import med, timed          # noqa: E402

SHAPES = ((1, 12, 8192), (16, 12, 16000))
FADE, PAUSE, PEAK = 40, 960, 0.9


def stock(rows, n, ramp, out, S, W):
    """the same sentences with stock torch: one host read of the lengths, one slice-add per word -> totals"""
    n_h = n.cpu().tolist()                                           # the host read
    t = torch.arange(rows.size(1), device=rows.device)
    peak = (rows.abs() * (t[None, :] < n[:, None])).amax(1)
    gain = torch.where(peak > 0, PEAK / peak, torch.ones_like(peak))
    out.zero_()
    F = ramp.numel()
    totals = []
    for s in range(S):
        at = 0
        for k in range(W):
            r = s * W + k
            m = n_h[r]
            w = torch.ones(m, device=rows.device)
            w[:F] = ramp
            w[m - F:] = ramp.flip(0)
            out[s, at:at + m] += rows[r, :m] * (gain[r] * w)
            at += m + (PAUSE if k + 1 < W else 0)
        totals.append(at)
    return totals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--says', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'prof_synth needs a GPU'
    from audiogan_amd import kernels as K
    from audiogan_amd import synth
    dev = torch.device('cuda')
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    say('joining words into sentences: us per call (device events around %d back-to-back calls), the forms alternating, '
        'medians of %d rounds' % (args.launches, args.rounds))
    i32 = torch.int32
    for S, W, L in SHAPES:
        rs = np.random.RandomState(7)
        R = S * W
        n_h = rs.randint(L // 2, L + 1, R)
        rows = torch.randn(R, L, device=dev) * 0.1
        rows *= (torch.arange(L, device=dev)[None, :] < torch.from_numpy(n_h).to(dev)[:, None])
        n = torch.from_numpy(n_h.astype(np.int32)).to(dev)
        off = torch.zeros(R, dtype=i32, device=dev)
        seg_row = torch.arange(R, dtype=i32, device=dev)
        join = torch.full((R,), PAUSE, dtype=i32, device=dev)
        sent_ptr = torch.arange(0, R + 1, W, dtype=i32, device=dev)
        ramp = K.join_ramp(FADE, dev)
        O_cap = W * L + (W - 1) * PAUSE
        out, out_s = torch.empty(S, O_cap, device=dev), torch.empty(S, O_cap, device=dev)
        out_len = torch.empty(S, dtype=torch.int64, device=dev)

        def facts():
            return K.join_facts(rows, off, n, PEAK)
        gain, bad = facts()

        def clips():
            K.join_clips(rows, off, n, gain, seg_row, join, sent_ptr, ramp, out, out_len, pause_max=PAUSE)

        def pair():
            g, _ = K.join_facts(rows, off, n, PEAK)
            K.join_clips(rows, off, n, g, seg_row, join, sent_ptr, ramp, out, out_len, pause_max=PAUSE)
        clips()
        name = K.lib.ag_last_kernel().decode()
        totals = stock(rows, n, ramp, out_s, S, W)
        torch.cuda.synchronize()
        assert out_len.tolist() == totals and not int(bad.sum()), 'the forms differ in their plans'
        assert torch.allclose(out, out_s, rtol=1e-5, atol=1e-7), 'the forms differ: %g' % float((out - out_s).abs().max())
        by = 4.0 * (float(n_h.sum()) + S * O_cap)
        t = dict(f=[], c=[], p=[], s=[])
        for r in range(args.rounds):
            t['f'].append(timed(facts, 5, args.launches) * 1e3)
            t['c'].append(timed(clips, 5, args.launches) * 1e3)
            t['p'].append(timed(pair, 5, args.launches) * 1e3)
            t['s'].append(timed(lambda: stock(rows, n, ramp, out_s, S, W), 2, max(1, args.launches // 10)) * 1e3)
            say('%d x %d words x %d samples, round %d: join_facts %8.2f us   join_clips %8.2f us   the pair %8.2f us   stock '
                '%10.2f us' % (S, W, L, r + 1, t['f'][-1], t['c'][-1], t['p'][-1], t['s'][-1]))
        say('%d sentence(s) x %d words x %d samples (out [%d, %d]): median ag_join_facts %.2f us, %s %.2f us = %.1f GB/s of %.1f MB '
            'read + written, the pair %.2f us with no host read;  the stock form (a host read of %d lengths, %d slice-adds) '
            '%.2f us = %.1f x the pair' % (S, W, L, S, O_cap, med(t['f']), name, med(t['c']), by / med(t['c']) / 1e3, by / 1e6,
                                          med(t['p']), R, R, med(t['s']), med(t['s']) / med(t['p'])))
        del rows, out, out_s

    import audiogan_amd as A
    torch.manual_seed(0)
    g = A.Generator(frame_size=256, embed_size=100, noise_size=100, state_size=1024, num_layers=1).to(dev)
    e_g = A.Embedder(output_size=100, char_embed_size=50, num_layers=1, num_chars=256).to(dev)
    v = synth.Voice(g, e_g, dev, max_samples=8192)
    text = 'the quick brown fox jumps over the lazy dog and runs away'
    v.say(text, seed=0)
    torch.cuda.synchronize()
    rates = []
    for r in range(args.rounds):
        t0, samples = time.perf_counter(), 0
        for i in range(args.says):
            wave, _ = v.say(text, seed=i)
            samples += wave.numel()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rates.append(samples / 8000.0 / dt)
        say('Voice.say, round %d: %d sentences of 12 words, %.2f s of audio in %.1f ms = %.0f s of audio per second'
            % (r + 1, args.says, samples / 8000.0, dt * 1e3, rates[-1]))
    say('Voice.say end to end (Embedder, one generate of 12 words up to 8192 samples, join, one host copy): median %.0f seconds '
        'of audio per second (rounds %s)' % (med(rates), ' '.join('%.0f' % x for x in rates)))
    K.check_persist_status(dev)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
