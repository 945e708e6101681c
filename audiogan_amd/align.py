"""Cutting transcribed utterances into words by template alignment - the step the reference's preprocessing hands to a forced
aligner (preprocess-fisher.py:100-149): the words of an utterance's transcript, each given by the cepstra of ONE recorded
take of it (its template), are laid out as a reference sequence, the utterance is time-warped onto it, and every word is cut
out where the warping path enters and leaves its template.

  path64(cep_a, n, cep_b, m)             the recursion and the tie rule of ag_dtw_align in float64 numpy -> (total, lo, hi)
  pause_frame(cep, nf)                   the one-frame pause model of an utterance
  reference_for(words, templates, cep)   [sil] w1 [sil] w2 .. wK [sil] -> (rows [F, 16], offsets, lengths)
  medoid(M)                              the row of a distance matrix with the smallest sum; the lowest index on a tie
  pick_templates(store, words)           per word the medoid of its first clips in a word store -> word -> cepstra
  align_utterances(waves, lens, ..)      melcep_frames, reference_for, one dtw_align launch per 64 utterances -> the cuts

THIS IS TEMPLATE ALIGNMENT, NOT AN HMM ALIGNER.  It cuts only words it has a template for - an utterance with any other word
is dropped whole, naming the word - and it is as good as the templates are: one speaker's takes align that speaker's speech
well and a stranger's less so.  Each cut carries its aligned mel-cepstral distance to the template in dB
(``evaluate.aligned_distance``'s number), so a caller can drop the poor ones.

The pause model is ONE column: the mean cepstrum of the utterance's quietest tenth of frames (by c[0], at least one frame).
The vertical step (i-1, j) repeats a column at the price of its local distance per frame, so one column absorbs a pause of
any length, and where two words touch the path passes it in one horizontal step; a pause model of several columns would force
that many frames between words that have none.

The cepstra come from ``kernels.melcep_frames``: a CUDA (HIP) device is needed, as in ``evaluate``; there is no host melcep in
the package.  With the cepstra at hand ``path64`` gives the path without a launch (``align_utterances(host_path=True)``)."""
import numpy as np

HOP, WIN = 128, 256          # melcep_frames' framing
MAX_FRAMES = 1024            # ag_dtw_align's capacity, either side
BATCH = 64                   # utterances per dtw_align launch
DIAG, UP, LEFT = 0, 1, 2     # the decision codes, in the order ties are settled


def require_device(device):
    """the torch.device alignment runs on; RuntimeError when it is not a CUDA (HIP) device"""
    import torch
    device = torch.device(device if device is not None else ('cuda' if torch.cuda.is_available() else 'cpu'))
    if device.type != 'cuda':
        raise RuntimeError('audiogan_amd.align: aligning needs a CUDA (HIP) device - the cepstra are computed by '
                           'kernels.melcep_frames and there is no host path; got %s' % device)
    return device


def frames(n):
    """frames melcep_frames makes of a clip of n samples"""
    n = int(n)
    return (n - WIN) // HOP + 1 if n >= WIN else 1


# ----------------------------------------------------------------------------------------------------------------------
# the recursion, in float64
# ----------------------------------------------------------------------------------------------------------------------
def path64(cep_a, n, cep_b, m):
    """cep_a [>= n, 16], cep_b [>= m, 16] (columns 1..12 are read; counts clamped to [1, rows]) -> (total, lo [m], hi [m]):
         d(i, j) = |a_i - b_j|,   D(0, 0) = 2 d,   D(i, j) = min(D(i-1, j-1) + 2 d, D(i-1, j) + d, D(i, j-1) + d)
    in float64, and the path from (n-1, m-1) back to (0, 0) that takes, at every cell, the first of (diagonal, (i-1, j),
    (i, j-1)) whose candidate equals the minimum.  lo[j] / hi[j]: the first / last row on the path in column j."""
    a, b = np.asarray(cep_a, dtype=np.float64), np.asarray(cep_b, dtype=np.float64)
    n, m = max(1, min(int(n), a.shape[0])), max(1, min(int(m), b.shape[0]))
    df = a[:n, None, 1:13] - b[None, :m, 1:13]
    d = np.sqrt((df * df).sum(-1))
    D = np.full((n + 1, m + 1), np.inf)          # D[i + 1, j + 1] = D(i, j); row 0 and column 0: no such cell
    code = np.full((n, m), LEFT, dtype=np.uint8)
    D[1, 1] = d[0, 0] + d[0, 0]
    for s in range(1, n + m - 1):                # cells of one anti-diagonal depend on the two before it only
        i = np.arange(max(0, s - m + 1), min(n - 1, s) + 1)
        j = s - i
        dd = d[i, j]
        cand = np.stack([D[i, j] + (dd + dd), D[i, j + 1] + dd, D[i + 1, j] + dd])          # DIAG, UP, LEFT
        D[i + 1, j + 1] = cand.min(0)
        code[i, j] = np.argmax(cand == cand.min(0), axis=0)          # the first that attains it
    code[0, :], code[:, 0] = LEFT, UP
    lo, hi = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
    i, j = n - 1, m - 1
    hi[j] = i
    while i or j:
        c = code[i, j]
        if c == UP:
            i -= 1
            continue
        lo[j] = i
        if c == DIAG:
            i -= 1
        j -= 1
        hi[j] = i
    lo[0] = 0
    return float(D[n, m]), lo, hi


# ----------------------------------------------------------------------------------------------------------------------
# references and templates
# ----------------------------------------------------------------------------------------------------------------------
def pause_frame(cep, nf=None):
    """cep [>= nf, 16] -> float32 [16]: the mean (in float64, rounded once) of the rows whose c[0] lies in the lowest tenth -
    the nf // 10 smallest, at least one; equal values in row order"""
    c = np.asarray(cep)
    c = c[:len(c) if nf is None else max(1, int(nf))]
    k = max(1, len(c) // 10)
    rows = np.argsort(c[:, 0], kind='stable')[:k]
    return c[rows].astype(np.float64).mean(0).astype(np.float32)


def reference_for(words, templates, cep, nf=None):
    """the reference sequence of one utterance: ``words`` its transcript, ``templates`` word -> cepstral rows [len, 16],
    ``cep`` / ``nf`` the utterance's own cepstra (for the pause column) -> (rows float32 [F, 16], offsets, lengths) with the
    layout [sil] w1 [sil] w2 .. wK [sil]: word k's template lies in columns offsets[k] .. offsets[k] + lengths[k] - 1 and
    F = K + 1 + sum(lengths)."""
    sil = pause_frame(cep, nf)[None, :]
    parts, offsets, lengths, at = [sil], [], [], 1
    for w in words:
        t = np.asarray(templates[w], dtype=np.float32)
        offsets.append(at)
        lengths.append(len(t))
        parts += [t, sil]
        at += len(t) + 1
    return np.concatenate(parts, 0), offsets, lengths


def reference_frames(words, templates):
    """F of ``reference_for`` without building it"""
    return len(words) + 1 + sum(len(templates[w]) for w in words)


def medoid(M):
    """M [k, k] pairwise distances -> the index of the row with the smallest sum; the lowest index wins a tie"""
    return int(np.argmin(np.asarray(M, dtype=np.float64).sum(1)))


def pick_templates(store, words, per_word=8, device=None):
    """``store``: word -> float32 [clips, maxlen] zero padded (ingest.load_store); ``words``: the words wanted -> word -> float32
    [frames, 16], the cepstral rows of the word's template, for every wanted word the store holds.  The template is the
    MEDOID of the word's first ``per_word`` clips in store order: the clip with the smallest sum of aligned distances
    total / (n + m) to the others (``medoid``); a word with one clip is its own template.  One melcep_frames launch over all
    candidate clips and one dtw_pairs launch over the ordered pairs inside every word."""
    import torch
    from . import kernels as K
    from .ingest import clip_length
    device = require_device(device)
    words = [w for w in dict.fromkeys(words) if w in store and len(store[w])]
    if not words:
        return {}
    clips, first = [], {}
    for w in words:
        first[w] = len(clips)
        clips += [np.asarray(c, dtype=np.float32)[:max(1, clip_length(c))] for c in store[w][:max(1, int(per_word))]]
    lens = np.array([len(c) for c in clips], dtype=np.int64)
    if frames(lens.max()) > MAX_FRAMES:
        raise ValueError('audiogan_amd.align: a template clip of %d samples has more than %d frames' % (lens.max(), MAX_FRAMES))
    buf = np.zeros((len(clips), int(lens.max())), dtype=np.float32)
    for r, c in enumerate(clips):
        buf[r, :len(c)] = c
    nf = torch.empty(len(clips), dtype=torch.int32, device=device)
    cep = K.melcep_frames(torch.from_numpy(buf).to(device), torch.from_numpy(lens).to(device), nframes=nf)
    count = {w: min(len(store[w]), max(1, int(per_word))) for w in words}
    ia = [first[w] + p for w in words for p in range(count[w]) for q in range(count[w])]
    ib = [first[w] + q for w in words for p in range(count[w]) for q in range(count[w])]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=device)          # noqa: E731
    tot = K.dtw_pairs(cep, nf, cep, nf, i32(ia), i32(ib)).double().cpu().numpy()
    nfh, ceph = nf.cpu().numpy().astype(np.int64), cep.cpu().numpy()
    out, at = {}, 0
    for w in words:
        k, r0 = count[w], first[w]
        M = tot[at:at + k * k].reshape(k, k) / (nfh[r0:r0 + k, None] + nfh[None, r0:r0 + k])
        at += k * k
        pick = r0 + medoid(M)
        out[w] = ceph[pick, :nfh[pick]].copy()
    return out


# ----------------------------------------------------------------------------------------------------------------------
# utterances -> cuts
# ----------------------------------------------------------------------------------------------------------------------
def word_span(lo, hi, offset, length, n_samples):
    """the samples [start, end) of a word whose template lies in columns offset .. offset + length - 1: from the first frame
    matched to its first column to the end of the last frame matched to its last"""
    return int(lo[offset]) * HOP, min(int(hi[offset + length - 1]) * HOP + WIN, int(n_samples))


def align_utterances(waves, lens, transcripts, templates, device=None, batch=BATCH, host_path=False):
    """``waves`` float32 [U, L] (numpy or tensor) at 8 kHz with their lengths ``lens`` [U]; ``transcripts``: per utterance the list
    of its words; ``templates``: word -> cepstral rows (``pick_templates``).  -> a list of U dicts
         cuts     [(word, start, end, db)] in transcript order: samples [start, end) of the utterance's row, and the aligned
                  mel-cepstral distance of the cut to the word's template in dB (evaluate.aligned_distance's number)
         dropped  None, or (reason, detail): 'no_template' with the first word that has none, 'too_long_to_align' when the
                  utterance or its reference has more than 1024 frames; ``cuts`` is then empty
    Route: ``kernels.melcep_frames`` of the utterances, ``reference_for`` each, ONE ``kernels.dtw_align`` launch per ``batch`` (at
    most 64) utterances, then one melcep_frames and one dtw_pairs launch score that batch's cuts.  ``host_path``: the path
    from ``path64`` on the same cepstra instead of the launch."""
    import torch
    from . import kernels as K
    from .evaluate import MCD_DB
    device = require_device(device)
    waves = waves if hasattr(waves, 'detach') else torch.from_numpy(np.ascontiguousarray(waves, dtype=np.float32))
    waves = waves.float().to(device)
    lens = np.asarray(lens.detach().cpu().numpy() if hasattr(lens, 'detach') else lens, dtype=np.int64).reshape(-1)
    U = int(waves.size(0))
    assert len(lens) == U == len(transcripts), (U, len(lens), len(transcripts))
    lens = np.clip(lens, 0, int(waves.size(1)))
    out = [dict(cuts=[], dropped=None) for _ in range(U)]
    todo = []
    for u, words in enumerate(transcripts):
        missing = [w for w in words if w not in templates]
        if missing:
            out[u]['dropped'] = ('no_template', missing[0])
        elif frames(lens[u]) > MAX_FRAMES or reference_frames(words, templates) > MAX_FRAMES:
            out[u]['dropped'] = ('too_long_to_align', '%d frames against %d' % (frames(lens[u]),
                                                                              reference_frames(words, templates)))
        elif words:
            todo.append(u)
    bank_words = sorted(set(w for u in todo for w in transcripts[u]))
    if bank_words:          # the templates as one bank for the scores
        Ft = max(len(templates[w]) for w in bank_words)
        bank = np.zeros((len(bank_words), Ft, 16), dtype=np.float32)
        for r, w in enumerate(bank_words):
            bank[r, :len(templates[w])] = templates[w]
        bank_nf = torch.tensor([len(templates[w]) for w in bank_words], dtype=torch.int32, device=device)
        bank, row_of = torch.from_numpy(bank).to(device), {w: r for r, w in enumerate(bank_words)}
    batch = max(1, min(int(batch), BATCH))
    for g0 in range(0, len(todo), batch):
        part = todo[g0:g0 + batch]
        rows = torch.tensor(part, dtype=torch.long, device=device)
        ln = lens[part]
        x = waves[rows, :max(1, int(ln.max()))].contiguous()
        nf = torch.empty(len(part), dtype=torch.int32, device=device)
        cep = K.melcep_frames(x, torch.from_numpy(ln).to(device), nframes=nf)
        ceph, nfh = cep.cpu().numpy(), nf.cpu().numpy()
        refs = [reference_for(transcripts[u], templates, ceph[r], nfh[r]) for r, u in enumerate(part)]
        Fb = max(len(ref) for ref, _, _ in refs)
        cep_b = np.zeros((len(part), Fb, 16), dtype=np.float32)
        for r, (ref, _, _) in enumerate(refs):
            cep_b[r, :len(ref)] = ref
        nf_b = np.array([len(ref) for ref, _, _ in refs], dtype=np.int32)
        if host_path:
            paths = [path64(ceph[r], nfh[r], cep_b[r], nf_b[r])[1:] for r in range(len(part))]
        else:
            _, lo, hi = K.dtw_align(cep, nf, torch.from_numpy(cep_b).to(device), torch.from_numpy(nf_b).to(device))
            lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
            paths = [(lo[r], hi[r]) for r in range(len(part))]
        spans = []          # (row of the batch, word, start, end)
        for r, u in enumerate(part):
            _, offsets, lengths = refs[r]
            for w, off, length in zip(transcripts[u], offsets, lengths):
                spans.append((r, w) + word_span(paths[r][0], paths[r][1], off, length, ln[r]))
        cl = np.array([z - a for _, _, a, z in spans], dtype=np.int64)
        cuts = torch.zeros(len(spans), max(1, int(cl.max())), dtype=torch.float32, device=device)
        for c, (r, _, a, z) in enumerate(spans):
            cuts[c, :z - a] = x[r, a:z]
        cnf = torch.empty(len(spans), dtype=torch.int32, device=device)
        ccep = K.melcep_frames(cuts, torch.from_numpy(cl).to(device), nframes=cnf)
        ib = torch.tensor([row_of[w] for _, w, _, _ in spans], dtype=torch.int32, device=device)
        ia = torch.arange(len(spans), dtype=torch.int32, device=device)
        tot = K.dtw_pairs(ccep, cnf, bank, bank_nf, ia, ib)
        db = (MCD_DB * tot.double() / (cnf + bank_nf[ib.long()]).double()).cpu().numpy()
        for c, (r, w, a, z) in enumerate(spans):
            out[part[r]]['cuts'].append((w, a, z, float(db[c])))
    return out
