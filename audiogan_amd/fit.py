"""Train from a word store to checkpoints: ``python -m audiogan_amd.fit --dataset words.npz --modelnamesave PREFIX --outer N``.

The command between ``audiogan_amd.ingest`` (WAV files -> a word store) and ``audiogan_amd.synth`` (a checkpoint and text -> a WAV
file): the reference's script as one call.  Its flags carry the reference's names and defaults (audiogan.py:554-579); the loop
it builds is INTEGRATION section 1 - ``Generator`` / ``Discriminator`` / two ``Embedder``s, two optimisers, ``dataset.dataloader``,
``loop.words_picker``, ``loop.TrainLoop`` - and everything opt-in since then hangs off a flag of its own: the device-resident store,
captured iterations, averaged weights, summaries, held-out evaluation, samples as WAV files and as sample sheets
(``sheet.SheetWriter``: one PNG per sampled minibatch, drawn on the device).

  build(args)      the constructed objects (models, optimisers, loaders, ``TrainLoop``, ...) without running anything
  main(argv)       parse, build, resume, run ``--outer`` passes; the last line on stdout is one JSON object

The reference loops ``while True``; here ``--outer`` says how many passes to run.  ``PREFIX-run.json`` records the parsed
arguments; ``synth`` needs none of it - it reads its shapes from the checkpoint."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

# (name, type, default): the reference's flags, audiogan.py:554-579
REFERENCE_FLAGS = (
    ('critic_iter', int, 100), ('rnng_layers', int, 1), ('rnnd_layers', int, 1), ('framesize', int, 200),
    ('noisesize', int, 100), ('gstatesize', int, 1024), ('dstatesize', int, 1024), ('batchsize', int, 32),
    ('dgradclip', float, 1), ('ggradclip', float, 0.1), ('dlr', float, 1e-4), ('glr', float, 1e-4),
    ('modelnamesave', str, ''), ('modelnameload', str, ''), ('loaditerations', int, 0), ('gencatchup', int, 1),
    ('dataset', str, 'dataset.h5'), ('embedsize', int, 100), ('minwordlen', int, 1), ('maxlen', int, 40000),
    ('noisescale', float, 0.01), ('g_optim', str, 'boundary_seeking'), ('require_acc', float, 0.5))
GRAPHED_NEEDS = "graphed=True needs stop='never' and a CUDA device"          # the loop's own words (loop.TrainLoop)


def _struct(text):
    """'17,8,16,8;9,4,16,8' -> [[17, 8, 16, 8], [9, 4, 16, 8]]"""
    try:
        return [[int(v) for v in layer.split(',')] for layer in text.split(';')]
    except ValueError:
        raise argparse.ArgumentTypeError('a structure is layers of integers: 17,8,16,8;9,4,16,8 - got %r' % text)


def parser():
    ap = argparse.ArgumentParser(prog='python -m audiogan_amd.fit', description=__doc__.split('\n\n')[0])
    ref = ap.add_argument_group("the reference's flags (audiogan.py:554-579)")
    for name, kind, default in REFERENCE_FLAGS:
        ref.add_argument('--' + name, type=kind, default=default)
    own = ap.add_argument_group('beyond the reference')
    own.add_argument('--outer', type=int, required=True, metavar='N', help='passes of the outer loop (the reference never stops)')
    own.add_argument('--device', default=None, help="default: 'cuda' if there is one")
    own.add_argument('--device-store', action='store_true', help='keep every clip on the device (dataset.DeviceWordStore)')
    own.add_argument('--graphed', action='store_true', help='capture the three iterations into graphs and replay them')
    own.add_argument('--fixed-critic-iter', type=int, default=None, metavar='K', help='K critic iterations a pass, no accuracy test')
    own.add_argument('--stop', choices=('draw', 'never'), default='draw', help="'never': fixed-length clips")
    own.add_argument('--dtype', choices=('f32', 'bf16'), default='f32', help='operand precision of the contractions')
    own.add_argument('--optim', choices=('rmsprop', 'adam'), default='rmsprop')
    own.add_argument('--ema', type=float, default=None, metavar='DECAY', help='average the generator weights (optim.EMA)')
    own.add_argument('--checkpoint-every', type=int, default=500, help='generator iterations between checkpoints (0: none)')
    own.add_argument('--sample-every', type=int, default=0, help='sample the fixed words every so many generator iterations')
    own.add_argument('--audio-every', type=int, default=0, help='write the samples as WAV files every so many')
    own.add_argument('--sheet-every', type=int, default=0, help='write the samples as one sample sheet (PNG) every so many')
    own.add_argument('--sheet-cols', type=int, default=8)
    own.add_argument('--sample-dir', default=None, help='default: PREFIX-samples')
    own.add_argument('--summary', default=None, metavar='FILE', help="the reference's scalars, one JSON line per iteration")
    own.add_argument('--eval-every', type=int, default=0, help='score held-out minibatches every so many generator iterations')
    own.add_argument('--eval-batches', type=int, default=4)
    own.add_argument('--aligned', action='store_true', help='evaluation: add the DTW-aligned mel-cepstral distance')
    own.add_argument('--crossed', action='store_true', help='evaluation: add diversity and word retrieval')
    own.add_argument('--pitch', action='store_true', help='evaluation: add F0 and voicing error along the aligned path')
    own.add_argument('--seed', type=int, default=0)
    shape = ap.add_argument_group('network shapes the reference fixes in its source')
    shape.add_argument('--gstruct', type=_struct, default=None, metavar='K,S,HID,OUT;..', help="the generator's conv stack")
    shape.add_argument('--dstruct', type=_struct, default=None, metavar='K,S,OUT;..', help="the critic's conv stack")
    shape.add_argument('--charembedsize', type=int, default=50)
    return ap


def parse(argv=None):
    """the parsed arguments, with every combination the loop would refuse refused here, in the loop's words"""
    ap = parser()
    a = ap.parse_args(argv)
    a.device = a.device or ('cuda' if torch.cuda.is_available() else 'cpu')
    cuda = torch.device(a.device).type == 'cuda'
    if a.outer < 0:
        ap.error('--outer %d: a number of passes' % a.outer)
    if a.graphed and not (a.stop == 'never' and cuda):
        ap.error('--graphed: ' + GRAPHED_NEEDS + ' (--stop never%s)' % ('' if cuda else ', --device cuda'))
    if a.device_store and not cuda:
        ap.error('--device-store keeps the clips on a GPU: --device %s has none' % a.device)
    if a.ema is not None and not 0.0 <= a.ema <= 1.0:
        ap.error('--ema: EMA: decay must lie in [0, 1], got %r' % (a.ema,))
    if a.fixed_critic_iter is not None and a.fixed_critic_iter < 0:
        ap.error('--fixed-critic-iter %d: a number of critic iterations' % a.fixed_critic_iter)
    for flag in ('sample_every', 'audio_every', 'sheet_every', 'eval_every', 'checkpoint_every', 'loaditerations'):
        if getattr(a, flag) < 0:
            ap.error('--%s %d: may not be negative' % (flag.replace('_', '-'), getattr(a, flag)))
    if a.sheet_every and not a.sample_every:
        a.sample_every = a.sheet_every          # sheets are drawn from the samples
    if a.sheet_every and a.sheet_every % a.sample_every:
        ap.error('--sheet-every %d: sheets are drawn from the samples, taken every %d (--sample-every): a multiple of it'
                 % (a.sheet_every, a.sample_every))
    if (a.aligned or a.crossed) and not a.eval_every:
        ap.error('--aligned / --crossed belong to the held-out evaluation: set --eval-every')
    if a.pitch and not a.eval_every:
        ap.error('--pitch belongs to the held-out evaluation: set --eval-every')
    if a.pitch and not a.aligned:
        ap.error('--pitch compares F0 along the time-warping path of the cepstra: set --aligned')
    if a.eval_every and a.eval_batches < 1:
        ap.error('--eval-batches %d: at least one held-out minibatch' % a.eval_batches)
    if a.loaditerations and not (a.modelnameload or a.modelnamesave):
        ap.error('--loaditerations %d needs --modelnameload (or --modelnamesave) to name the checkpoint' % a.loaditerations)
    if (a.sample_every or a.audio_every) and not a.modelnamesave and a.sample_dir is None:
        ap.error('samples need a place: --sample-dir, or --modelnamesave PREFIX (then PREFIX-samples)')
    return a


def _sample_dir(a):
    if a.sample_dir is not None:
        return a.sample_dir
    return a.modelnamesave + '-samples' if a.modelnamesave else None


def build(a):
    """``a``: what ``parse`` returns.  -> a namespace of everything INTEGRATION section 1 constructs: g, d, e_g, e_d, opt_g, opt_d,
    ema, summary, evaluator, sheets, loop (the ``TrainLoop``), store, keys_train, keys_valid, maxlen, first (the first held-out
    minibatch: its words are the fixed sample words), sample_dir.  Nothing has run: no iteration, no file."""
    import audiogan_amd as A
    from . import dataset, evaluate, kernels as K, loop, optim, sheet, summary
    dev = torch.device(a.device)
    np.random.seed(a.seed)
    torch.manual_seed(a.seed)
    K.set_precision(a.dtype)
    B, frame = a.batchsize, a.framesize
    extra_g = dict(struct=a.gstruct) if a.gstruct else {}
    extra_d = dict(cnn_struct=a.dstruct) if a.dstruct else {}
    g = A.Generator(frame_size=frame, noise_size=a.noisesize, state_size=a.gstatesize, embed_size=a.embedsize,
                    num_layers=a.rnng_layers, **extra_g).to(dev)
    d = A.Discriminator(state_size=a.dstatesize, embed_size=a.embedsize, num_layers=a.rnnd_layers, **extra_d).to(dev)
    e_g = A.Embedder(a.embedsize, char_embed_size=a.charembedsize).to(dev)
    e_d = A.Embedder(a.embedsize, char_embed_size=a.charembedsize).to(dev)
    opt_g = optim.make_optimizer(list(g.parameters()) + list(e_g.parameters()), a.optim, a.glr)          # audiogan.py:690-694
    opt_d = optim.make_optimizer(list(d.parameters()) + list(e_d.parameters()), a.optim, a.dlr)
    ema = optim.EMA(opt_g, decay=a.ema) if a.ema is not None else None

    largs = types.SimpleNamespace(conditional=True, dataset=a.dataset, minwordlen=a.minwordlen, subset=None, amplitudes=0,
                                  device_store=a.device if a.device_store else None)
    largs.dataset = dataset._open(a.dataset)          # (opened once: the loader takes the mapping as it takes the path)
    n_words = len(dataset._valid_keys(list(largs.dataset.keys()), largs))
    if n_words < 10:
        raise ValueError('audiogan_amd.fit: %d words of at least %d characters in the store: the loader trains on 9 words in 10 '
                         '(dataset.py:98-110) and would have none left - at least 10 words' % (n_words, a.minwordlen))
    store, maxlen, gen_train, gen_valid, keys_train, keys_valid = dataset.dataloader(B, largs, maxlen=a.maxlen or None,
                                                                                     frame_size=frame)
    # held-out minibatches BEFORE the training loader's first next(): both draw from the global numpy generator
    heldout = [next(gen_valid) for _ in range(max(1, a.eval_batches if a.eval_every else 1))]
    first = heldout[0]
    sample_words = (np.asarray(first[5]), np.asarray(first[6]))          # audiogan.py:672-681: cseq_fixed, clen_fixed
    pick = loop.words_picker(dataset, B, maxlen, store, keys_train, largs, frame_size=frame)
    sm = summary.Summary(dev, path=a.summary) if a.summary else None
    ev = None
    if a.eval_every:
        ev = evaluate.Evaluator(g, d, e_g, e_d, heldout, B, maxlen, dev, batches=len(heldout), seed=a.seed, ema=ema,
                                path=(a.summary + '.eval') if a.summary else None, aligned=a.aligned, crossed=a.crossed,
                                pitch=a.pitch)
    sdir = _sample_dir(a)
    sheets = sheet.SheetWriter(sdir, every=a.sheet_every or 1, cols=a.sheet_cols) if sdir is not None else None
    sampling = bool(a.sample_every or a.audio_every)
    lp = loop.TrainLoop(
        g, d, e_g, e_d, opt_g, opt_d, gen_train, pick, B, maxlen, dev, noisescale=a.noisescale, critic_iter=a.critic_iter,
        require_acc=a.require_acc, gencatchup=a.gencatchup, dgradclip=a.dgradclip, ggradclip=a.ggradclip, g_optim=a.g_optim,
        checkpoint_every=a.checkpoint_every, checkpoint_prefix=a.modelnamesave or None, fixed_critic_iter=a.fixed_critic_iter,
        stop='never' if a.stop == 'never' else None, check=not a.graphed, graphed=a.graphed,
        sample_every=a.sample_every, sample_words=sample_words if sampling else None, sample_seed=a.seed,
        on_sample=sheets if a.sheet_every else None, sample_dir=sdir if a.audio_every else None, audio_every=a.audio_every,
        summary=sm, ema=ema, evaluator=ev, eval_every=a.eval_every)
    if sheets is not None:
        sheets.samples = lp.L          # every sheet of the run at one geometry: generate() returns rows as wide as its longest sample
    return types.SimpleNamespace(args=a, g=g, d=d, e_g=e_g, e_d=e_d, opt_g=opt_g, opt_d=opt_d, ema=ema, summary=sm, evaluator=ev,
                                 sheets=sheets, loop=lp, store=store, keys_train=keys_train, keys_valid=keys_valid, maxlen=maxlen,
                                 first=first, sample_dir=sdir, device=dev)


def real_sheet(s):
    """the first held-out minibatch's real clips as ``<sample dir>/real-sheet.png`` (the reference logs them as ``real_plot`` at
    iteration 0, audiogan.py:672-675) -> the path"""
    samples, lengths = s.first[2], np.asarray(s.first[3])
    wave = torch.from_numpy(np.ascontiguousarray(np.asarray(samples), dtype=np.float32)).to(s.device)
    return s.sheets.write('real-sheet.png', wave, torch.from_numpy(lengths.astype(np.int64)).to(s.device))


def resume(s, prefix, iteration):
    """``TrainLoop.resume`` from the checkpoint ``prefix`` wrote at generator iteration ``iteration`` (it need not be the prefix
    this run saves under) -> the checkpoint's ``extra``"""
    lp = s.loop
    keep, lp.prefix = lp.prefix, prefix
    try:
        return lp.resume(iteration)
    finally:
        lp.prefix = keep


def _snapshot(a, sample_dir):
    """{path: modification time} of what a run may write: PREFIX-*, the sample folder, the summary files"""
    out = []
    if a.modelnamesave:
        folder, stem = os.path.split(os.path.abspath(a.modelnamesave))
        if os.path.isdir(folder):
            out += [os.path.join(folder, n) for n in sorted(os.listdir(folder)) if n.startswith(stem + '-')]
    if sample_dir and os.path.isdir(sample_dir):
        out += [os.path.join(os.path.abspath(sample_dir), n) for n in sorted(os.listdir(sample_dir))]
    if a.summary:
        out += [os.path.abspath(p) for p in (a.summary, a.summary + '.eval')]
    return {p: os.stat(p).st_mtime_ns for p in out if os.path.isfile(p)}


def main(argv=None):
    a = parse(argv)
    s = build(a)
    lp = s.loop
    before = _snapshot(a, s.sample_dir)
    if a.modelnamesave:
        os.makedirs(os.path.dirname(os.path.abspath(a.modelnamesave)), exist_ok=True)
        with open(a.modelnamesave + '-run.json', 'w') as f:
            json.dump({k: v for k, v in sorted(vars(a).items())}, f, indent=1)
            f.write('\n')
    if a.loaditerations:
        resume(s, a.modelnameload or a.modelnamesave, a.loaditerations)
    elif s.sheets is not None and a.sheet_every:
        real_sheet(s)
    start = (lp.dis_iter, lp.gen_iter)
    lp.run(a.outer)
    if a.modelnamesave and a.checkpoint_every and lp.gen_iter % a.checkpoint_every and lp.gen_iter > start[1]:
        every, lp.checkpoint_every = lp.checkpoint_every, 1          # the state the run ends in is kept, whatever the period
        try:
            lp._maybe_checkpoint()
        finally:
            lp.checkpoint_every = every
    row = None
    if a.summary and os.path.exists(a.summary):
        with open(a.summary) as f:
            lines = f.read().splitlines()
        row = json.loads(lines[-1]) if lines else None
    files = [p for p, t in _snapshot(a, s.sample_dir).items() if before.get(p) != t]
    result = dict(dis_iter=lp.dis_iter, gen_iter=lp.gen_iter, dis_iter_run=lp.dis_iter - start[0],
                  gen_iter_run=lp.gen_iter - start[1], summary=row, evaluation=lp.eval_log[-1] if lp.eval_log else None,
                  files=files)
    print(json.dumps(result))
    sys.stdout.flush()
    return 0


if __name__ == '__main__':
    sys.exit(main())
