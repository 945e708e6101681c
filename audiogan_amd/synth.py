"""From a checkpoint and a line of text to a WAV file - the exit that matches the entrance ``ingest`` built.  The reference has
no inference path (audiogan.py trains and logs); this is beyond the reference and touches nothing of the training path.

  models_from_checkpoint(prefix, it)  the Generator / GRUGenerator and the Embedder rebuilt from the shapes in the files
  Voice(g, e_g, device, ...)          say_batch(sentences) / say(text): words generated in chunks, joined on the device
  join_plan(n, join)                  where each word of a sentence starts: the integer plan of ag_join_clips
  facts_host / join_host              the two launches in numpy fp32, bit for bit: the path without a GPU
  render(path, wave, sr_out, fmt)     resample (audio.resample: ag_resample_poly on a GPU) and write PCM16 or float32

A sentence is its words' clips one after the other: a pause of ``pause_ms`` between them, or an overlap of ``overlap_ms``; the
first and last ``fade_ms`` of every word are shaped by a raised-sine ramp, every word is scaled to the peak ``peak``.  The
clips' lengths stay on the device: ``kernels.join_facts`` and ``kernels.join_clips`` (ag_join_facts, ag_join_clips) read them
there, and one host copy after the launches brings back the totals.

  python -m audiogan_amd.synth --checkpoint PREFIX --iteration N (--text "..." | --text-file FILE) --out OUT.wav
         [--rate 16000] [--format pcm16|float32] [--seed 0] [--pause-ms 120] [--fade-ms 5] [--overlap-ms 0]
         [--max-seconds 2.0] [--peak 0.9 | --no-normalise] [--trim] [--no-ema] [--marks-out TSV] [--device D]"""
import argparse
import os
import re
import sys
import warnings

import numpy as np
import torch

from . import audio, checkpoint, dataset

CHUNK = 64          # words generated per call of g.generate


# ------------------------------------------------------------------------------------------------------------------
# the rule: the plan in integers, the two launches in numpy fp32
# ------------------------------------------------------------------------------------------------------------------
def join_plan(n, join):
    """``n``: the lengths of a sentence's segments, ``join`` one entry per segment (the last is ignored): >= 0 a pause of that
    many samples after the segment, < 0 an overlap of min(-join, n_k // 2, n_{k+1} // 2) samples with the next.
    -> (starts, total): st_0 = 0, st_{k+1} = st_k + n_k + pause or st_k + n_k - overlap, total = st_last + n_last (0 for an
    empty sentence).  Python integers; the model of ag_join_clips' prologue and the source of ``Voice``'s marks."""
    n = [int(v) for v in n]
    starts, at = [], 0
    for k, nk in enumerate(n):
        starts.append(at)
        at += nk
        if k + 1 < len(n):
            j = int(join[k])
            at += j if j >= 0 else -min(-j, nk // 2, n[k + 1] // 2)
    return starts, at


def _windows(off, n, L_in):
    off = np.clip(np.asarray(off, dtype=np.int64), 0, L_in)
    return off, np.clip(np.asarray(n, dtype=np.int64), 0, L_in - off)


def facts_host(wave, off, n, target=0.0):
    """ag_join_facts on the host -> (gain float32 [R], bad int32 [R])"""
    wave = np.asarray(wave, dtype=np.float32)
    R, L_in = wave.shape
    off, n = _windows(off, n, L_in)
    gain, bad = np.ones(R, dtype=np.float32), np.zeros(R, dtype=np.int32)
    for r in range(R):
        x = wave[r, off[r]:off[r] + n[r]]
        if not np.isfinite(x).all():
            gain[r], bad[r] = 0.0, 1
        elif target > 0 and len(x):
            peak = np.abs(x).max()
            if peak > 0:
                with np.errstate(over='ignore'):
                    gain[r] = np.float32(target) / peak
    return gain, bad


def join_host(wave, off, n, gain, seg_row, join, sent_ptr, ramp, O_cap):
    """ag_join_clips on the host, sample by sample as the launch takes them (the segment of each output found by a search of
    the starts), in numpy fp32: the same rule, the same bits -> (out float32 [S, O_cap], out_len int64 [S])"""
    wave, gain, ramp = (np.asarray(a, dtype=np.float32) for a in (wave, gain, ramp))
    seg_row, join, sent_ptr = (np.asarray(a, dtype=np.int64) for a in (seg_row, join, sent_ptr))
    R, L_in = wave.shape
    off, n = _windows(off, n, L_in)
    F, S = len(ramp), len(sent_ptr) - 1
    out, out_len = np.zeros((S, int(O_cap)), dtype=np.float32), np.zeros(S, dtype=np.int64)

    def term(rows, o, m, i, on):
        """x * (gain * w) of sample i of the segments (rows, o, m), where ``on``; anything where not"""
        i = np.where(on, i, 0)
        m1 = np.where(on, m, 1)
        f = np.minimum(F, m1 // 2)
        j = m1 - 1 - i
        w = np.ones(len(i), dtype=np.float32)
        head, tail = on & (i < f), on & (i >= f) & (j < f)
        fs = np.maximum(f, 1)
        if F:
            w[head] = ramp[(i * F // fs)[head]]
            w[tail] = ramp[(j * F // fs)[tail]]
        x = wave[np.where(on, rows, 0), np.where(on, o + i, 0)] if L_in else np.zeros(len(i), dtype=np.float32)
        return x * (gain[np.where(on, rows, 0)] * w)

    for s in range(S):
        ks = np.arange(sent_ptr[s], sent_ptr[s + 1])
        rows = seg_row[ks]
        live = (rows >= 0) & (rows < R)
        rows = np.where(live, rows, 0)
        o, m = (off[rows], np.where(live, n[rows], 0)) if R else (rows * 0, rows * 0)
        st, total = join_plan(m, join[ks])
        out_len[s] = total
        T = min(total, int(O_cap))
        if T <= 0:
            continue
        st = np.asarray(st, dtype=np.int64)
        t = np.arange(T, dtype=np.int64)
        kb = np.searchsorted(st, t, side='right') - 1          # the last k with st_k <= t
        ka = np.maximum(kb - 1, 0)
        has_b = t - st[kb] < m[kb]
        has_a = (kb > 0) & (t - st[ka] < m[ka])
        with np.errstate(all='ignore'):
            vb = term(rows[kb], o[kb], m[kb], t - st[kb], has_b)
            va = term(rows[ka], o[ka], m[ka], t - st[ka], has_a)
            out[s, :T] = np.where(has_a & has_b, va + vb, np.where(has_b, vb, np.where(has_a, va, np.float32(0))))
    return out, out_len


# ------------------------------------------------------------------------------------------------------------------
# the modules back from a checkpoint
# ------------------------------------------------------------------------------------------------------------------
def _shape(sd, key, dims, where):
    if key not in sd:
        raise ValueError('%s: no tensor %r: not a generator / embedder state_dict of this package' % (where, key))
    shp = tuple(sd[key].shape)
    if len(shp) != dims:
        raise ValueError('%s: %r has shape %r, expected %d axes' % (where, key, shp, dims))
    return shp


def _indices(sd, pattern):
    rx = re.compile(pattern)
    return sorted({int(m.group(1)) for m in (rx.match(k) for k in sd) if m})


def infer_generator_args(sd, embed_size, where='gen'):
    """-> ('lstm' | 'gru', constructor arguments) from the shapes of a Generator / GRUGenerator state_dict"""
    fs, S = _shape(sd, 'proj.module.weight_v', 2, where)
    layers = _indices(sd, r'rnn\.(\d+)\.module\.weight_ih_v$')
    if layers != list(range(len(layers))) or not layers:
        raise ValueError('%s: recurrent layers %r: expected rnn.0 .. rnn.<n-1>' % (where, layers))
    rows, fin = _shape(sd, 'rnn.0.module.weight_ih_v', 2, where)
    if rows == 4 * S:
        kind = 'lstm'
    elif rows == 3 * S:
        kind = 'gru'
        if len(layers) != 1:
            raise ValueError('%s: a GRU front (rnn.0.module.weight_ih_v %r) with %d layers: GRUGenerator has one'
                             % (where, (rows, fin), len(layers)))
    else:
        raise ValueError('%s: rnn.0.module.weight_ih_v has shape %r: %d rows are neither 4 nor 3 times the state size %d'
                         % (where, (rows, fin), rows, S))
    noise = fin - fs - embed_size
    if noise < 0:
        raise ValueError('%s: rnn.0.module.weight_ih_v has shape %r: %d inputs less a frame of %d and an embedding of %d '
                         'leave a noise size of %d' % (where, (rows, fin), fin, fs, embed_size, noise))
    blocks = _indices(sd, r'dense_res_gen\.(\d+)\.module\.conv\.weight_v$')
    if blocks != list(range(len(blocks))):
        raise ValueError('%s: trunk blocks %r: expected dense_res_gen.0 .. <n-1>' % (where, blocks))
    struct, cin = [], 1
    for i in blocks:
        ck_key, dk_key = 'dense_res_gen.%d.module.conv.weight_v' % i, 'dense_res_gen.%d.module.deconv.weight_v' % i
        hidden, c_in, ck = _shape(sd, ck_key, 3, where)
        h2, cout, dk = _shape(sd, dk_key, 3, where)
        stride = dk // 2
        if ck != 2 * stride + 1 or dk != ck - 1:
            raise ValueError('%s: %r has shape %r and %r %r: a conv kernel of %d is not 2 * stride + 1 with the stride %d of a '
                             'deconv kernel of %d' % (where, ck_key, (hidden, c_in, ck), dk_key, (h2, cout, dk), ck, stride, dk))
        if c_in != cin or h2 != hidden:
            raise ValueError('%s: %r has shape %r and %r %r: expected %d input channels and equal hidden sizes'
                             % (where, ck_key, (hidden, c_in, ck), dk_key, (h2, cout, dk), cin))
        struct.append((ck, stride, hidden, cout))
        cin += cout
    last = 'dense_res_gen.%d.module.weight_v' % len(blocks)
    if _shape(sd, last, 3, where) != (1, cin, 3):
        raise ValueError('%s: %r has shape %r, expected %r' % (where, last, tuple(sd[last].shape), (1, cin, 3)))
    args = dict(frame_size=fs, embed_size=embed_size, noise_size=noise, state_size=S, struct=struct)
    if kind == 'lstm':
        args['num_layers'] = len(layers)
    return kind, args


def infer_embedder_args(sd, where='eg'):
    """-> the constructor arguments of an Embedder from the shapes of its state_dict"""
    num_chars, ce = _shape(sd, 'embed.module.weight', 2, where)
    rows, H = _shape(sd, 'rnn.weight_hh_l0', 2, where)
    ih = _shape(sd, 'rnn.weight_ih_l0', 2, where)
    if rows != 4 * H or ih != (4 * H, ce):
        raise ValueError('%s: rnn.weight_hh_l0 has shape %r and rnn.weight_ih_l0 %r: expected (4 H, H) and (4 H, %d)'
                         % (where, (rows, H), ih, ce))
    layers = _indices(sd, r'rnn\.weight_ih_l(\d+)$')
    if layers != list(range(len(layers))):
        raise ValueError('%s: recurrent layers %r: expected l0 .. l<n-1>' % (where, layers))
    return dict(output_size=2 * H, char_embed_size=ce, num_layers=len(layers), num_chars=num_chars)


def models_from_checkpoint(prefix, iteration, use_ema=True, device='cuda', allow_pickle=False):
    """-> (g, e_g, info): the generator and its Embedder as ``checkpoint.save`` wrote them, rebuilt with the constructor
    arguments their tensors' shapes imply and loaded with ``strict=True``.  ``use_ema``: the averaged weights (the ``genema`` /
    ``egema`` files) when they exist, else the plain ones with one warning; ``info['weights']`` says which ('ema' / 'plain'),
    ``info['kind']`` 'lstm' or 'gru', ``info['generator']`` / ``info['embedder']`` the arguments.  Whatever cannot be mapped
    is refused with the offending key and shape."""
    from . import modules
    ema = bool(use_ema)
    if ema and not all(os.path.exists(checkpoint._path(prefix, r, iteration)) for r in ('genema', 'egema')):
        warnings.warn('audiogan_amd.synth: %s holds no averaged weights (genema / egema): using the plain ones'
                      % checkpoint._path(prefix, 'gen', iteration))
        ema = False
    sds = {}
    for role in ('gen', 'eg'):
        path = checkpoint._path(prefix, checkpoint._EMA_ROLES[role] if ema else role, iteration)
        obj = checkpoint._read(path, allow_pickle)
        sds[role] = (obj.state_dict() if isinstance(obj, torch.nn.Module) else obj), path
    eargs = infer_embedder_args(*sds['eg'])
    kind, gargs = infer_generator_args(sds['gen'][0], eargs['output_size'], sds['gen'][1])
    g = (modules.GRUGenerator if kind == 'gru' else modules.Generator)(**gargs).to(device)
    e_g = modules.Embedder(**eargs).to(device)
    checkpoint.load(prefix, iteration, g=g, e_g=e_g, strict=True, allow_pickle=allow_pickle, use_ema=ema)
    g.eval()
    e_g.eval()
    return g, e_g, dict(weights='ema' if ema else 'plain', kind=kind, generator=gargs, embedder=eargs)


# ------------------------------------------------------------------------------------------------------------------
# the voice
# ------------------------------------------------------------------------------------------------------------------
class Voice(object):
    """``g``: anything with ``generate(c, length=, z=, u=)`` -> (wave [B, <= L], _, _, length [B]), ``_frame_size`` and
    ``_noise_size``; ``e_g``: any callable (cseq int64 [B, C], clen int64 [B]) -> [B, embed].  ``max_samples``: the longest
    word (rounded up to whole frames); ``fade_ms`` the ramp at either end of a word, ``pause_ms`` the silence between words -
    or, with ``overlap_ms`` > 0, how far neighbours overlap; ``peak``: every word is scaled to this peak (None or 0: left as
    generated); ``trim``: ``audio.activity`` (options: the dict ``activity``) cuts each word to its first-to-last active
    stretch before the join.  Rates in Hz at ``sr``, the models' rate."""

    def __init__(self, g, e_g, device, max_samples=16000, fade_ms=5.0, pause_ms=120.0, overlap_ms=0.0, peak=0.9, trim=False,
                 activity=None, sr=8000):
        from . import kernels as K
        self.g, self.e_g, self.device, self.sr = g, e_g, torch.device(device), int(sr)
        self.frame = int(g._frame_size)
        self.frames = max(1, -(-int(max_samples) // self.frame))
        self.fade = int(round(fade_ms * sr / 1000.0))
        if not 0 <= self.fade <= K.JOIN_MAX_FADE:
            raise ValueError('audiogan_amd.synth: a fade of %d samples (%g ms): 0 .. %d' % (self.fade, fade_ms, K.JOIN_MAX_FADE))
        self.join = -int(round(overlap_ms * sr / 1000.0)) if overlap_ms > 0 else int(round(pause_ms * sr / 1000.0))
        self.peak = float(peak) if peak else 0.0
        self.trim, self.activity = bool(trim), dict(activity or {})
        self.chunk = CHUNK
        emb = getattr(getattr(e_g, 'embed', None), 'module', None)
        self.num_chars = int(emb.weight.shape[0]) if emb is not None else int(getattr(e_g, 'num_chars', 256))

    @classmethod
    def from_checkpoint(cls, prefix, iteration, use_ema=True, device='cuda', allow_pickle=False, **options):
        g, e_g, info = models_from_checkpoint(prefix, iteration, use_ema, device, allow_pickle)
        v = cls(g, e_g, device, **options)
        v.info = info
        return v

    def _words(self, sentences):
        out = []
        for s in sentences:
            words = s.split() if isinstance(s, str) else [str(w) for w in s]
            for w in words:
                if not w or any(ord(ch) >= self.num_chars for ch in w):
                    raise ValueError('audiogan_amd.synth: the word %r holds a character outside the embedder\'s %d' %
                                     (w, self.num_chars))
            out.append(words)
        return out

    @torch.no_grad()
    def _rows(self, flat, seed):
        """every word generated, ``self.chunk`` at a time -> (rows [R, L_in] on the device, n int32 [R] on the device).  z and
        the stop uniforms of ALL words are drawn at once from a private generator: where the chunks fall changes nothing."""
        dev, R, T = self.device, len(flat), self.frames
        L_in = T * self.frame
        gen = torch.Generator().manual_seed(int(seed))
        z = torch.randn(R, T, int(self.g._noise_size), generator=gen)
        u = torch.rand(T, R, generator=gen)
        rows = torch.zeros(R, L_in, dtype=torch.float32, device=dev)
        n = torch.zeros(R, dtype=torch.int32, device=dev)
        width = max([len(w) for w in flat] + [1])
        for c0 in range(0, R, self.chunk):
            part = flat[c0:c0 + self.chunk]
            cseq = torch.from_numpy(np.stack([dataset.word_to_seq(w, width) for w in part]).astype(np.int64)).to(dev)
            clen = torch.tensor([len(w) for w in part], dtype=torch.int64, device=dev)
            c = self.e_g(cseq, clen).float()
            wave, _, _, length = self.g.generate(c, length=L_in, z=z[c0:c0 + len(part)].to(dev),
                                                 u=u[:, c0:c0 + len(part)].contiguous().to(dev))
            rows[c0:c0 + len(part), :wave.size(1)] = wave[:, :L_in]
            n[c0:c0 + len(part)] = length.to(dev).clamp(0, L_in).to(torch.int32)
        return rows, n

    def say_batch(self, sentences, seed=0):
        """``sentences``: strings (split on whitespace) or lists of words; an empty one is allowed.  -> (out float32 [S, O_cap]
        on the device, out_len int64 [S] numpy, marks): sentence s is out[s, :out_len[s]], marks[s] a list of (word, start
        sample, end sample).  The same sentences and seed give the same bits; no global RNG moves."""
        from . import kernels as K
        words = self._words(sentences)
        flat = [w for ws in words for w in ws]
        S, R, dev = len(words), len(flat), self.device
        most = max([len(ws) for ws in words] + [0])
        if most > K.JOIN_MAX_SEGMENTS:
            raise ValueError('audiogan_amd.synth: a sentence of %d words: at most %d' % (most, K.JOIN_MAX_SEGMENTS))
        rows, n = self._rows(flat, seed)
        L_in = rows.size(1)
        off = torch.zeros(R, dtype=torch.int32, device=dev)
        if self.trim and R:
            o_h, n_h = np.zeros(R, dtype=np.int32), n.cpu().numpy().copy()
            for r, seg in enumerate(audio.activity(rows, lens=n_h, sr=self.sr, device=dev, **self.activity)):
                if seg is not None and len(seg):          # (no stretch: the whole row; a NaN: join_facts reports it)
                    o_h[r], n_h[r] = seg[0, 0], seg[-1, 1] - seg[0, 0]
            off, n = torch.from_numpy(o_h).to(dev), torch.from_numpy(n_h).to(dev)
        sent_ptr = np.concatenate([[0], np.cumsum([len(ws) for ws in words])]).astype(np.int32)
        seg_row = np.arange(R, dtype=np.int32)
        join = np.full(R, self.join, dtype=np.int32)
        pause = max(self.join, 0)
        O_cap = (most * L_in + max(most - 1, 0) * pause + 3) // 4 * 4
        ramp = K.join_ramp(self.fade, dev)
        if dev.type == 'cuda':
            gain, bad = K.join_facts(rows, off, n, self.peak)
            out = torch.empty(S, O_cap, dtype=torch.float32, device=dev)
            _, out_len = K.join_clips(rows, off, n, gain, torch.from_numpy(seg_row).to(dev), torch.from_numpy(join).to(dev),
                                      torch.from_numpy(sent_ptr).to(dev), ramp, out, pause_max=pause)
            back = torch.cat([out_len, bad.long(), off.long(), n.long()]).cpu().numpy()          # the one host copy
            out_len, bad, off_h, n_h = back[:S], back[S:S + R], back[S + R:S + 2 * R], back[S + 2 * R:]
        else:
            wave_h, off_h, n_h = rows.numpy(), off.numpy(), n.numpy()
            gain, bad = facts_host(wave_h, off_h, n_h, self.peak)
            out, out_len = join_host(wave_h, off_h, n_h, gain, seg_row, join, sent_ptr, ramp.numpy(), O_cap)
            out = torch.from_numpy(out)
        for r in np.flatnonzero(bad):
            raise ValueError('audiogan_amd.synth: the generator gave a NaN or an infinity for the word %r (word %d)' % (flat[r], r))
        _, n_w = _windows(off_h, n_h, L_in)
        marks = []
        for s, ws in enumerate(words):
            k0 = int(sent_ptr[s])
            st, total = join_plan(n_w[k0:k0 + len(ws)], join[k0:k0 + len(ws)])
            assert total == int(out_len[s]), (s, total, int(out_len[s]))
            marks.append([(w, st[k], st[k] + int(n_w[k0 + k])) for k, w in enumerate(ws)])
        return out, np.asarray(out_len, dtype=np.int64).copy(), marks

    def say(self, text, seed=0):
        """-> (wave float32 [total] on the device, marks) of one sentence"""
        out, out_len, marks = self.say_batch([text], seed)
        return out[0, :int(out_len[0])], marks[0]


def render(path, wave, sr_out=16000, fmt='pcm16', sr=8000):
    """``wave`` (1-D, at ``sr`` Hz) resampled to ``sr_out`` by ``audio.resample`` - the launch for 16 / 22.05 / 44.1 / 48 kHz on
    a GPU, its host path with its warning for a pair the launch refuses - and written as ``fmt`` ('pcm16' / 'float32').
    -> the number of samples written"""
    wave = wave.detach() if hasattr(wave, 'detach') else torch.from_numpy(np.asarray(wave, dtype=np.float32))
    wave = wave.reshape(-1).float()
    if int(sr_out) != int(sr) and wave.numel():
        y, counts = audio.resample(wave, sr, sr_out)
        wave = y[0, :int(counts[0])]
    audio.write_wav(path, wave, sr=int(sr_out), fmt=fmt)
    return int(wave.numel())


def write_marks(tsv, paths, marks, sr=8000):
    """``path<TAB>word<TAB>start_s<TAB>end_s`` per word, a time as ``ingest.write_cuts`` writes it ('%.6f' % ((sample + 0.5) /
    sr), at the models' rate): ``ingest --manifest`` cuts the words back out of a rendering at that rate.  -> lines"""
    lines = ['%s\t%s\t%.6f\t%.6f\n' % (os.path.abspath(p), w, (a + 0.5) / sr, (z + 0.5) / sr)
             for p, ms in zip(paths, marks) for w, a, z in ms]
    with open(tsv, 'w', encoding='utf-8') as f:
        f.write('# path, word, start_s, end_s: the words of each sentence (audiogan_amd.synth --marks-out)\n')
        f.writelines(lines)
    return len(lines)


def main(argv=None, voice=None):
    """``voice``: a ready ``Voice`` in place of the one the checkpoint options describe (the tests' hook)"""
    ap = argparse.ArgumentParser(prog='python -m audiogan_amd.synth', description=__doc__.split('\n\n')[0])
    ap.add_argument('--checkpoint', metavar='PREFIX', required=voice is None)
    ap.add_argument('--iteration', type=int, required=voice is None)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--text')
    src.add_argument('--text-file', metavar='FILE', help='one sentence per line: OUT-000.wav, OUT-001.wav, ..')
    ap.add_argument('--out', required=True, metavar='OUT.wav')
    ap.add_argument('--rate', type=int, default=16000)
    ap.add_argument('--format', choices=('pcm16', 'float32'), default='pcm16')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--pause-ms', type=float, default=120.0)
    ap.add_argument('--fade-ms', type=float, default=5.0)
    ap.add_argument('--overlap-ms', type=float, default=0.0)
    ap.add_argument('--max-seconds', type=float, default=2.0, help='the longest word')
    nrm = ap.add_mutually_exclusive_group()
    nrm.add_argument('--peak', type=float, default=0.9)
    nrm.add_argument('--no-normalise', action='store_true')
    ap.add_argument('--trim', action='store_true')
    ap.add_argument('--no-ema', action='store_true')
    ap.add_argument('--marks-out', metavar='TSV')
    ap.add_argument('--device', default=None)
    a = ap.parse_args(argv)
    if voice is None:
        device = a.device or ('cuda' if torch.cuda.is_available() else 'cpu')
        voice = Voice.from_checkpoint(a.checkpoint, a.iteration, use_ema=not a.no_ema, device=device,
                                      max_samples=int(round(a.max_seconds * 8000)), fade_ms=a.fade_ms, pause_ms=a.pause_ms,
                                      overlap_ms=a.overlap_ms, peak=None if a.no_normalise else a.peak, trim=a.trim)
    if a.text_file:
        with open(a.text_file, encoding='utf-8') as f:
            sentences = [line.rstrip('\r\n') for line in f]
        root, ext = os.path.splitext(a.out)
        paths = ['%s-%03d%s' % (root, i, ext) for i in range(len(sentences))]
    else:
        sentences, paths = [a.text], [a.out]
    out, out_len, marks = voice.say_batch(sentences, seed=a.seed)
    for s, path in enumerate(paths):
        render(path, out[s, :int(out_len[s])], sr_out=a.rate, fmt=a.format, sr=voice.sr)
    if a.marks_out:
        write_marks(a.marks_out, paths, marks, sr=voice.sr)
    return 0


if __name__ == '__main__':
    sys.exit(main())
