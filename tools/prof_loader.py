"""What does a loader minibatch cost on the host, from the loader's ``next()`` to the step's static tensors, with the host
loader and with the device-resident word store (dataset.DeviceWordStore), and what do the two launches of the store cost?

  * per minibatch, at (B 64, 8192 samples, frame 256), (B 64, 40000, 200 - the reference's --maxlen) and (B 32, 40000, 200),
    over a synthetic store of ``--words`` x ``--per-word`` noise clips (2000 by default):
      host loader     ``next(gen)`` (dataset.pick_words: float64 rows), the float32 cast and padding of TrainLoop._host_pair,
                      train.Feeder.stage (pinned copy, upload) and feed (device copy)            - host milliseconds
      device loader   ``next(gen)`` (ids only), Feeder(clips=...).stage (B ids) and feed (one ag_clip_gather) - host milliseconds
    host clock around ``--batches`` minibatches ending in a synchronise, the two alternating, medians of ``--rounds`` rounds;
  * the gather launch alone: device events around ``--launches`` back-to-back launches, microseconds and TB/s of clip samples
    read plus rows written; ag_clip_facts over the whole store the same way;
  * the eager and the captured TrainLoop at the C2 widths (tools/prof_eval.py's models) from either loader, in the same run:
    wall milliseconds per pass (2 critic + 1 generator iteration, ending in a synchronise) and the loop's host milliseconds
    per pass in the loader and in staging (``host_ms['loader']`` / ``['stage']``; the eager loop has no such counters: the
    time inside TrainLoop._real is taken instead).

    python tools/prof_loader.py [--out profiles/loader_device.txt]
"""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.prof_eval import med, timed          # noqa: E402

SHAPES = ((64, 8192, 256), (64, 40000, 200), (32, 40000, 200))


def loaders(ds, B, maxlen, frame, dev, store=None):
    from audiogan_amd import dataset as D
    out = []
    for device_store in (None, dev):
        args = types.SimpleNamespace(conditional=True, dataset=ds if device_store is None else (store or ds), minwordlen=1,
                                     subset=None, amplitudes=0)
        if device_store is not None:
            args.device_store = device_store
        np.random.seed(5)
        out.append(D.dataloader(B, args, maxlen=maxlen, frame_size=frame))
    return out


def loops(B, dev, graphed):
    """TrainLoops at the C2 widths from the host loader and from the device loader (tools/prof_eval.py: setup)"""
    import audiogan_amd as A
    from audiogan_amd import dataset as D
    from audiogan_amd import loop, optim
    frame, maxlen = 256, 8192
    words = ['word%02d' % i for i in range(40)]
    ds = D.SyntheticWordDataset(words, n_per_word=4, min_len=maxlen // 3, max_len=maxlen, kind='noise', seed=3)
    out = []
    for h5, ml, gen_train, _, keys_train, _ in loaders(ds, B, maxlen, frame, dev):
        torch.manual_seed(0)
        g = A.Generator(frame_size=frame, embed_size=100, noise_size=100, state_size=1024, num_layers=1).to(dev)
        d = A.Discriminator(state_size=1024, embed_size=100, num_layers=1).to(dev)
        e_g, e_d = (A.Embedder(output_size=100, char_embed_size=50, num_layers=1, num_chars=256).to(dev) for _ in range(2))
        opt_g = optim.make_optimizer(list(g.parameters()) + list(e_g.parameters()), 'rmsprop', 1e-4)
        opt_d = optim.make_optimizer(list(d.parameters()) + list(e_d.parameters()), 'rmsprop', 1e-4)
        args = types.SimpleNamespace(conditional=True, dataset=ds, minwordlen=1, subset=None, amplitudes=0)
        pick = loop.words_picker(D, B, ml, h5, keys_train, args, frame_size=frame)
        lp = loop.TrainLoop(g, d, e_g, e_d, opt_g, opt_d, gen_train, pick, B, ml, dev, fixed_critic_iter=2, gencatchup=1,
                            stop='never', checkpoint_every=0, check=False, graphed=graphed, host=False)
        lp.real_ms = 0.0
        if not graphed:
            real = lp._real

            def timed_real(real=real, lp=lp):
                t0 = time.perf_counter()
                r = real()
                lp.real_ms += (time.perf_counter() - t0) * 1e3
                return r
            lp._real = timed_real
        out.append(lp)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batches', type=int, default=10)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--words', type=int, default=40)
    ap.add_argument('--per-word', type=int, default=50)
    ap.add_argument('--batch', type=int, default=64, help='the TrainLoops\' batch size')
    ap.add_argument('--no-loops', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'prof_loader needs a GPU'
    from audiogan_amd import dataset as D
    from audiogan_amd import kernels as K
    from audiogan_amd import train
    dev = torch.device('cuda')
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    say('loader minibatches: host ms per minibatch from next() to the static tensors (host clock around %d minibatches ending '
        'in a synchronise), launches in us (device events around %d back-to-back launches); medians of %d alternating rounds'
        % (args.batches, args.launches, args.rounds))
    made = {}
    for B, maxlen, frame in SHAPES:
        if maxlen not in made:
            made.clear()
            words = ['word%02d' % i for i in range(args.words)]
            ds = D.SyntheticWordDataset(words, n_per_word=args.per_word, min_len=maxlen // 3, max_len=maxlen, kind='noise', seed=3)
            t0 = time.perf_counter()
            store = D.DeviceWordStore(ds, dev)
            torch.cuda.synchronize()
            made[maxlen] = (ds, store, (time.perf_counter() - t0) * 1e3)
        ds, store, build_ms = made[maxlen]
        (_, ml, hgen, _, _, _), (_, _, dgen, _, _, _) = loaders(ds, B, maxlen, frame, dev, store)
        L = (ml + frame - 1) // frame * frame
        st_h = dict(real=torch.zeros(B, L, device=dev), real_len=torch.zeros(B, dtype=torch.long, device=dev))
        st_d = dict(real=torch.zeros(B, L, device=dev), real_len=torch.zeros(B, dtype=torch.long, device=dev))
        f_h = train.Feeder(st_h, keys=['real', 'real_len'])
        f_d = train.Feeder(st_d, keys=['real', 'real_len'], clips=('real', 'real_len'))

        def host_batch():
            _, _, samples, lengths, _, _, _ = next(hgen)
            x = np.zeros((B, L), dtype=np.float32)
            n = min(L, samples.shape[1])
            x[:, :n] = samples[:, :n]
            f_h.stage(dict(real=x, real_len=np.ascontiguousarray(lengths, dtype=np.int64)))
            f_h.feed()

        def device_batch():
            f_d.stage(dict(real=next(dgen)[2]))
            f_d.feed()

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.batches):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.batches

        state = np.random.get_state()          # (both loaders draw from the global numpy RNG: the same picks for the check)
        host_batch()
        np.random.set_state(state)
        device_batch()
        torch.cuda.synchronize()
        assert torch.equal(st_h['real'], st_d['real']) and torch.equal(st_h['real_len'], st_d['real_len']), 'the loaders differ'
        batch = next(dgen)[2]
        out, ln = torch.empty(B, L, device=dev), torch.empty(B, dtype=torch.long, device=dev)
        batch.gather(out, ln)
        name = K.lib.ag_last_kernel().decode()
        by = 4.0 * (float(np.minimum(store.n[batch.ids], L).sum()) + B * L)
        # the launches as nodes of one captured graph: at ~10 us a call the Python wrapper, not the kernel, paces launches
        # issued one by one
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, capture_error_mode='thread_local'):
            for _ in range(args.launches):
                batch.gather(out, ln)
        t = dict(h=[], d=[], g=[], q=[], f=[])
        for r in range(args.rounds):
            t['h'].append(wall(host_batch))
            t['d'].append(wall(device_batch))
            t['g'].append(timed(lambda: batch.gather(out, ln), 5, args.launches) * 1e3)
            t['q'].append(timed(graph.replay, 2, 5) * 1e3 / args.launches)
            t['f'].append(timed(lambda: K.clip_facts(store.bank, store.start, store.cap), 2, max(1, args.launches // 10)) * 1e3)
            say('B %d, %d samples, frame %d, round %d: host loader %8.3f ms   device loader %8.3f ms   gather %8.2f us issued '
                'one by one, %8.2f us as graph nodes   clip_facts %9.2f us'
                % (B, maxlen, frame, r + 1, t['h'][-1], t['d'][-1], t['g'][-1], t['q'][-1], t['f'][-1]))
        bank_by = 4.0 * store.bank.numel()
        say('B %d, %d samples, frame %d (rows of %d): median host loader %.3f ms, device loader %.3f ms per minibatch (%.1f x);  '
            '%s %.2f us issued one by one, %.2f us as %d nodes of a replayed graph = %.2f TB/s of %.1f MB read + written;  '
            'ag_clip_facts over %d clips (%.0f MB) %.1f us = %.2f TB/s;  the store was built (packed, uploaded, facts read '
            'back) in %.0f ms'
            % (B, maxlen, frame, L, med(t['h']), med(t['d']), med(t['h']) / med(t['d']), name, med(t['g']), med(t['q']),
               args.launches, by / med(t['q']) / 1e6, by / 1e6, store.n_clips, bank_by / 1e6, med(t['f']),
               bank_by / med(t['f']) / 1e6, build_ms))
        del graph, f_h, f_d, st_h, st_d, out
    made.clear()
    if not args.no_loops:
        say('TrainLoop at the C2 widths, B %d, 8192 samples, frame 256: wall ms per pass (2 critic + 1 generator iteration) around '
            '%d passes ending in a synchronise; host ms per pass in the loader and in staging' % (args.batch, args.passes))
        for graphed in (False, True):
            kind = 'captured' if graphed else 'eager'
            pair = loops(args.batch, dev, graphed)
            for lp in pair:
                for _ in range(3):
                    lp.outer()          # (captured: two eager warm-up passes, the captures, one replayed pass)
            t = ([], [])
            h0 = [dict(lp.host_ms, real=lp.real_ms, **({'f_' + k: v for k, v in lp._feeder.host_ms.items()} if graphed else {}))
                  for lp in pair]
            for r in range(args.rounds):
                for i, lp in enumerate(pair):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.passes):
                        lp.outer()
                    torch.cuda.synchronize()
                    t[i].append((time.perf_counter() - t0) * 1e3 / args.passes)
                say('%s, round %d: host loader %8.2f ms per pass   device loader %8.2f ms per pass' % (kind, r + 1, t[0][-1], t[1][-1]))
            n = float(args.rounds * args.passes)
            for i, (lp, which) in enumerate(zip(pair, ('host loader', 'device loader'))):
                if graphed:
                    extra = 'host_ms per pass: loader %.3f, stage %.3f, inputs %.3f' % tuple(
                        (lp.host_ms[k] - h0[i][k]) / n for k in ('loader', 'stage', 'inputs'))
                    extra += ';  of stage: %.3f waiting for the staging slot\'s previous replay, %.3f filling pinned memory' % tuple(
                        (lp._feeder.host_ms[k] - h0[i]['f_' + k]) / n for k in ('sync', 'pin'))
                else:
                    extra = 'host ms per pass inside TrainLoop._real (3 minibatches): %.3f' % ((lp.real_ms - h0[i]['real']) / n)
                say('%s TrainLoop, %s: median %.2f ms per pass (rounds %s);  %s'
                    % (kind, which, med(t[i]), ' '.join('%.2f' % v for v in t[i]), extra))
            K.check_persist_status(dev)
            del pair
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
