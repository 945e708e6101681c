"""Audio out and in.

Out: what the reference's summaries write with ``librosa.output.write_wav(wav_file, sample, sr=8000)``
(audiogan.py:655-667) - a mono WAV file of 32-bit IEEE floats (format tag 3) - with the standard library only.

In: what the reference's preprocessing reads with ``librosa.load(wav, sr=8000)`` (preprocess.py:24,
preprocess-fisher.py:232): ``read_wav`` (RIFF WAV, standard library and numpy), and a polyphase windowed-sinc resampler to
the models' 8 kHz - ``resample_bank`` designs the filter bank on the host in float64, ``resample64`` is the rule in float64
numpy (the path without a GPU, and the reference of every test), ``resample`` runs it on the device through
``kernels.resample_poly`` (ag_resample_poly), in chunks.

Where the words are: ``activity`` finds the active stretches of rows of 8 kHz samples by short-time energy (the reference cuts
words by a forced alignment, preprocess-fisher.py:145-146, or keeps loud windows, preprocess.py:25-27) - ``activity_rule`` is
the rule on the host, ``activity64`` the path without a GPU, and on the device ``kernels.frame_power`` and
``kernels.activity_segments`` (ag_frame_power, ag_activity_segments) run it.

Pitch: ``pitch64`` is the rule of ``kernels.pitch_frames`` (ag_pitch_frames) in float64 numpy - per frame the first strong peak
of the normalised cross-correlation - the arbiter of its tests and the path without a GPU (``evaluate.pitch_cents`` refines
its lags to cents)."""
import math
import struct
import warnings

import numpy as np

WAVE_FORMAT_PCM = 1
WAVE_FORMAT_IEEE_FLOAT = 3
WAVE_FORMAT_EXTENSIBLE = 0xFFFE


def write_wav(path, samples, sr=8000, fmt='float32'):
    """write ``samples`` (1-D, any float array or tensor) to ``path`` as a mono WAV at ``sr`` Hz: 32-bit floats (format tag 3)
    by default; ``fmt='pcm16'``: 16-bit PCM (format tag 1), clip(rint(x * 32767), -32768, 32767)"""
    if hasattr(samples, 'detach'):
        samples = samples.detach().cpu().numpy()
    if fmt == 'pcm16':
        x = np.asarray(samples, dtype=np.float32).reshape(-1).astype(np.float64)
        data = np.clip(np.rint(x * 32767.0), -32768, 32767).astype('<i2').tobytes()
        fmt_chunk = struct.pack('<HHIIHH', WAVE_FORMAT_PCM, 1, int(sr), int(sr) * 2, 2, 16)
        body = b'WAVE' + b'fmt ' + struct.pack('<I', len(fmt_chunk)) + fmt_chunk + b'data' + struct.pack('<I', len(data)) + data
        with open(path, 'wb') as f:
            f.write(b'RIFF' + struct.pack('<I', len(body)) + body)
        return
    if fmt != 'float32':
        raise ValueError("audiogan_amd: write_wav writes 'float32' or 'pcm16', not %r" % (fmt,))
    data = np.ascontiguousarray(np.asarray(samples, dtype=np.float32).reshape(-1)).astype('<f4').tobytes()
    channels, bits = 1, 32
    block = channels * bits // 8
    # RIFF header, the 'fmt ' chunk of a non-PCM format (cbSize = 0), a 'fact' chunk (required for non-PCM data), 'data'
    fmt = struct.pack('<HHIIHHH', WAVE_FORMAT_IEEE_FLOAT, channels, int(sr), int(sr) * block, block, bits, 0)
    fact = struct.pack('<I', len(data) // block)
    body = (b'WAVE' + b'fmt ' + struct.pack('<I', len(fmt)) + fmt + b'fact' + struct.pack('<I', len(fact)) + fact +
            b'data' + struct.pack('<I', len(data)) + data)
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', len(body)) + body)


def read_wav(path):
    """-> (data [frames, channels], sr).  ``data`` is int16 for 16-bit PCM and float32 for everything else: 8-bit unsigned
    as (v - 128) / 128, 24-bit / 2^23, 32-bit / 2^31, IEEE float 32 / 64 unchanged in value.  Format tags 1, 3 and 0xFFFE
    (extensible: the tag is the first two bytes of the sub-format); unknown chunks are skipped, the pad byte after an
    odd-sized chunk is honoured, a ``data`` size of 0 or 0xFFFFFFFF means "to the end of the file", and a truncated file
    gives its whole frames.  Anything else raises ValueError naming the file and the reason."""
    def bad(why):
        return ValueError('%s: %s' % (path, why))

    with open(path, 'rb') as f:
        raw = f.read()
    if len(raw) < 12 or raw[:4] != b'RIFF' or raw[8:12] != b'WAVE':
        raise bad('not a RIFF/WAVE file')
    pos, fmt = 12, None
    while pos + 8 <= len(raw):
        cid, size = raw[pos:pos + 4], struct.unpack_from('<I', raw, pos + 4)[0]
        pos += 8
        if cid == b'fmt ':
            if size < 16 or pos + 16 > len(raw):
                raise bad('a fmt chunk of %d bytes' % size)
            tag, channels, sr, _, block, bits = struct.unpack_from('<HHIIHH', raw, pos)
            if tag == WAVE_FORMAT_EXTENSIBLE:
                if size < 26 or pos + 26 > len(raw):
                    raise bad('an extensible fmt chunk of %d bytes' % size)
                tag = struct.unpack_from('<H', raw, pos + 24)[0]
            fmt = (tag, channels, sr, bits)
        elif cid == b'data':
            if fmt is None:
                raise bad('no fmt chunk before data')
            tag, channels, sr, bits = fmt
            if tag not in (WAVE_FORMAT_PCM, WAVE_FORMAT_IEEE_FLOAT):
                raise bad('format tag 0x%04X is compressed or unknown (PCM and IEEE float are read)' % tag)
            if channels == 0:
                raise bad('zero channels')
            kinds = {(WAVE_FORMAT_PCM, 8): 'u1', (WAVE_FORMAT_PCM, 16): '<i2', (WAVE_FORMAT_PCM, 24): None,
                     (WAVE_FORMAT_PCM, 32): '<i4', (WAVE_FORMAT_IEEE_FLOAT, 32): '<f4', (WAVE_FORMAT_IEEE_FLOAT, 64): '<f8'}
            if (tag, bits) not in kinds:
                raise bad('%d bits per sample with format tag %d' % (bits, tag))
            if size == 0 or size == 0xFFFFFFFF:
                size = len(raw) - pos
            body = raw[pos:pos + size]
            frame = channels * bits // 8
            frames = len(body) // frame
            body = body[:frames * frame]
            if (tag, bits) == (WAVE_FORMAT_PCM, 24):
                b3 = np.frombuffer(body, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
                v = b3[:, 0] | (b3[:, 1] << 8) | (b3[:, 2] << 16)
                v = np.where(v >= 1 << 23, v - (1 << 24), v)
                data = (v.astype(np.float64) / float(1 << 23)).astype(np.float32)
            else:
                v = np.frombuffer(body, dtype=kinds[(tag, bits)])
                if bits == 16:
                    data = v.astype(np.int16)
                elif bits == 8:
                    data = ((v.astype(np.float64) - 128.0) / 128.0).astype(np.float32)
                elif tag == WAVE_FORMAT_PCM:
                    data = (v.astype(np.float64) / float(1 << 31)).astype(np.float32)
                else:
                    data = v.astype(np.float32)
            return np.ascontiguousarray(data.reshape(frames, channels)), int(sr)
        pos += size + (size & 1)
    raise bad('no data chunk' if fmt is not None else 'no fmt chunk')


# ------------------------------------------------------------------------------------------------------------------
# resampling: y[N] = sum_t bank[p, t] x[base - half + t],  base = (N M) div L,  p = (N M) mod L
# ------------------------------------------------------------------------------------------------------------------
_BANKS = {}


def _bank64(L, M, zeros, beta, rolloff):
    fc = rolloff * min(1.0, L / M)
    W = zeros / fc
    half = int(math.ceil(W))
    t = np.arange(2 * half + 1, dtype=np.float64)[None, :]
    p = np.arange(L, dtype=np.float64)[:, None]
    u = t - half - p / L
    inside = np.abs(u) <= W
    win = np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (u / W) ** 2))) / np.i0(beta)
    return half, np.where(inside, fc * np.sinc(fc * u) * win, 0.0)


def resample_bank(sr_in, sr_out=8000, zeros=16, beta=8.0, rolloff=0.95, device='cpu'):
    """-> (L, M, half, bank [L, 2 half + 1] fp32 on ``device``): the Kaiser-windowed sinc at cutoff
    fc = rolloff min(1, L / M) (in units of half the input rate), ``zeros`` zero crossings a side, W = zeros / fc,
    half = ceil(W), bank[p, t] = fc sinc(fc u) I0(beta sqrt(1 - (u / W)^2)) / I0(beta) for |u| <= W = zeros / fc,
    u = t - half - p / L.  Evaluated in float64, rounded once to fp32; cached per (rates, parameters, device)."""
    import torch
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in <= 0 or sr_out <= 0:
        raise ValueError('audiogan_amd: sample rates %d -> %d' % (sr_in, sr_out))
    g = math.gcd(sr_in, sr_out)
    L, M = sr_out // g, sr_in // g
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    key = (L, M, int(zeros), float(beta), float(rolloff))
    if key + ('cpu',) not in _BANKS:
        half, bank = _bank64(L, M, int(zeros), float(beta), float(rolloff))
        _BANKS[key + ('cpu',)] = (half, torch.from_numpy(bank.astype(np.float32)))
    if key + (str(device),) not in _BANKS:
        half, bank = _BANKS[key + ('cpu',)]
        _BANKS[key + (str(device),)] = (half, bank.to(device))
    half, bank = _BANKS[key + (str(device),)]
    return L, M, half, bank


def out_count(n, L, M):
    """samples out of ``n`` frames in: ceil(n L / M)"""
    return (int(n) * L + M - 1) // M


def mono32(x):
    """[n] or [n, C], int16 or float -> fp32 [n]: the launch's rule - channels added in order in fp32, times fp32(1 / C);
    int16 values then times 2^-15"""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[:, None]
    is16 = x.dtype == np.int16
    x = x.astype(np.float32)
    s = x[:, 0].copy()
    for c in range(1, x.shape[1]):
        s += x[:, c]
    s *= np.float32(1.0) / np.float32(x.shape[1])
    if is16:
        s *= np.float32(2.0 ** -15)
    return s


_BLOCK = 1 << 14          # rows of one phase gathered at a time in resample64


def resample_rule64(x, bank, L, M, out_start=0, n_out=None, in_start=0):
    """the rule in float64 on given values: ``x`` [n] holds frames in_start .. in_start + n - 1 (zero elsewhere), ``bank``
    [L, taps]; -> float64 y[out_start .. out_start + n_out - 1] (default: all ceil(n L / M) of a signal starting at 0).
    Python integers and int64 throughout; vectorised per phase."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    bank = np.asarray(bank, dtype=np.float64)
    taps = bank.shape[1]
    half = (taps - 1) // 2
    n = x.shape[0]
    if n_out is None:
        n_out = out_count(n, L, M)
    y = np.zeros(n_out, dtype=np.float64)
    if n_out == 0:
        return y
    first = (int(out_start) * M) // L - half                      # the lowest frame any output reads
    last = ((int(out_start) + n_out - 1) * M) // L + half
    pad = np.zeros(last - first + 1, dtype=np.float64)            # frames first .. last
    lo, hi = max(first, int(in_start)), min(last + 1, int(in_start) + n)
    if hi > lo:
        pad[lo - first:hi - first] = x[lo - int(in_start):hi - int(in_start)]
    for j0 in range(min(L, n_out)):                                # outputs j0, j0 + L, ..: one phase each
        N0 = int(out_start) + j0
        p = (N0 * M) % L
        cnt = (n_out - j0 + L - 1) // L
        start = (N0 * M) // L - half - first                       # row k starts at start + k M
        for k0 in range(0, cnt, _BLOCK):
            k1 = min(cnt, k0 + _BLOCK)
            seg = pad[start + k0 * M:start + (k1 - 1) * M + taps]
            rows = np.lib.stride_tricks.as_strided(seg, shape=(k1 - k0, taps), strides=(M * seg.strides[0], seg.strides[0]),
                                                   writeable=False)
            y[j0 + k0 * L:j0 + k1 * L:L] = rows @ bank[p]
    return y


def resample64(x, sr_in, sr_out=8000):
    """``x`` [n] or [n, C] (int16 or float) -> float64 [ceil(n L / M)]: the rule of ``resample_bank`` in float64 numpy on
    the fp32-rounded bank and the fp32 mono samples the launch forms.  ``sr_in == sr_out`` returns the mono samples."""
    mono = mono32(x)
    if int(sr_in) == int(sr_out):
        return mono.astype(np.float64)
    L, M, half, bank = resample_bank(sr_in, sr_out)
    return resample_rule64(mono, bank.numpy(), L, M)


def _as_rows(x):
    """-> (tensor or array [B, n, C], is_tensor)"""
    is_t = hasattr(x, 'detach')
    if not is_t:
        x = np.asarray(x)
    nd = x.dim() if is_t else x.ndim
    if nd == 1:
        x = x[None, :, None]
    elif nd == 2:
        x = x[:, :, None]
    elif nd != 3:
        raise ValueError('audiogan_amd: resample takes [n], [B, n] or [B, n, C], got %d axes' % nd)
    return x, is_t


def resample(x, sr_in, sr_out=8000, lens=None, device=None, chunk=1 << 22):
    """``x`` [n], [B, n] or [B, n, C], numpy or tensor, int16 or float; ``lens``: frames per row (default n) ->
    (y [B, ceil(n L / M)] float32 on the device used, counts [B] int64 numpy = ceil(lens L / M)); y is zero at and past a
    row's count.  On a CUDA device, when ``kernels.resample_ok`` admits the rate pair, ag_resample_poly runs in launches of at
    most ``chunk`` output samples, each fed the window of frames it reads (a host source is uploaded window by window: an
    hour-long file needs no hour-long device buffer).  Otherwise ``resample64`` on the host - with one warning naming the
    rate pair when a GPU was there and the launch refused it."""
    import torch
    x, is_t = _as_rows(x)
    B, n, C = (int(s) for s in x.shape)
    if device is None:
        device = x.device if is_t and x.is_cuda else ('cuda' if torch.cuda.is_available() else 'cpu')
    device = torch.device(device)
    is16 = (x.dtype == torch.int16) if is_t else (x.dtype == np.int16)
    if not is16:
        x = x.float() if is_t else x.astype(np.float32, copy=False)
    ln = np.full(B, n, dtype=np.int64) if lens is None else np.clip(
        (lens.detach().cpu().numpy() if hasattr(lens, 'detach') else np.asarray(lens)).astype(np.int64).reshape(B), 0, n)
    g = math.gcd(int(sr_in), int(sr_out))
    L, M = int(sr_out) // g, int(sr_in) // g
    counts = (ln * L + M - 1) // M
    n_max = out_count(n, L, M)
    on_gpu = device.type == 'cuda'
    if on_gpu and L != M:
        from . import kernels as K
        _, _, half, bank = resample_bank(sr_in, sr_out, device=device)
        if K.resample_ok(L, M, bank.size(1), C, 1 if is16 else 0):
            y = torch.empty(B, n_max, dtype=torch.float32, device=device)
            ln_t = torch.from_numpy(ln)
            chunk = max(1, int(chunk))
            for o0 in range(0, n_max, chunk):
                o1 = min(n_max, o0 + chunk)
                lo = max(0, (o0 * M) // L - half)
                hi = max(lo, min(n, ((o1 - 1) * M) // L + half + 1))
                part = x[:, lo:hi]
                part = part.to(device) if is_t else torch.from_numpy(np.ascontiguousarray(part)).to(device)
                K.resample_poly(part, (ln_t - lo).clamp_(0, hi - lo).to(device), bank, L, M, dst=y[:, o0:o1], in_start=lo,
                                out_start=o0)
            if lens is not None:          # (the launch writes all n_max entries: past a row's count, the filter's tail)
                y.masked_fill_(torch.arange(n_max, device=device)[None, :] >= torch.from_numpy(counts).to(device)[:, None], 0.0)
            return y, counts
        warnings.warn('audiogan_amd: ag_resample_poly refuses %d -> %d Hz (L %d, %d taps: a bank over 64 KB); resampling '
                      'on the host in float64' % (sr_in, sr_out, L, bank.size(1)))
    xh = x.detach().cpu().numpy() if is_t else x
    y = np.zeros((B, n_max), dtype=np.float32)
    for b in range(B):
        if ln[b]:
            y[b, :counts[b]] = resample64(xh[b, :ln[b]], sr_in, sr_out)
    return torch.from_numpy(y).to(device), counts


# ------------------------------------------------------------------------------------------------------------------
# activity: an energy gate relative to the loudest frame (the rule of include/audiogan_hip.h: ag_activity_segments)
# ------------------------------------------------------------------------------------------------------------------
def activity_params(sr=8000, top_db=40.0, floor_db=-80.0, win_ms=25.0, hop_ms=10.0, min_gap_ms=300.0, min_run_ms=50.0,
                    pad_ms=30.0):
    """the options of ``activity`` as the launches take them: win = round(sr win_ms / 1000), hop likewise, the three durations
    in frames as ceil(ms / hop_ms), ratio = fp32(10^(-top_db / 10)), floor = fp32(10^(floor_db / 10))"""
    win, hop = int(round(sr * win_ms / 1000.0)), int(round(sr * hop_ms / 1000.0))
    if not 1 <= hop <= win <= 4096:
        raise ValueError('audiogan_amd: a window of %d samples at a hop of %d: 1 <= hop <= win <= 4096' % (win, hop))
    frames = lambda ms: int(math.ceil(ms / float(hop_ms)))          # noqa: E731
    return dict(win=win, hop=hop, min_gap=frames(min_gap_ms), min_run=frames(min_run_ms), pad=frames(pad_ms),
                ratio=np.float32(10.0 ** (-top_db / 10.0)), floor=np.float32(10.0 ** (floor_db / 10.0)))


def frame_count(n, hop):
    """frames of a row of ``n`` samples: ceil(n / hop) - every frame that starts inside the row; the last ones run past its
    end and read zeros there, so a word at the very end of a file is still seen"""
    return (np.asarray(n, dtype=np.int64) + hop - 1) // hop


def _order_keys(p):
    """fp32 -> int32 in the order of the values, -0 below +0 (its own inverse on the bits)"""
    i = np.ascontiguousarray(p, dtype=np.float32).view(np.int32)
    return i ^ ((i >> 31) & np.int32(0x7fffffff))


def activity_rule(power, nf, lens, ratio, floor, min_gap, min_run, pad, win, hop):
    """THE RULE on the host, run by run.  ``power`` [B, F] fp32, ``nf`` [B] frames and ``lens`` [B] samples per row ->
    (segs, count int32 [B], pmax fp32 [B]); segs[b] is an int64 array [count, 2] of (start, end) samples, None for a row with
    a NaN or an infinity (count -1, pmax NaN).  All in integers but for thr = max(fp32(pmax ratio), floor):
      1. active[f] = power[f] > thr, pmax the row's largest power (0 for an empty row);
      2. an inactive run strictly between two active frames and shorter than ``min_gap`` becomes active;
      3. then an active run shorter than ``min_run`` becomes inactive;
      4. a run of frames [a, b) becomes samples [max(0, (a - pad) hop), min(len, (b - 1 + pad) hop + win)); ranges that overlap
         or touch become one."""
    power = np.asarray(power, dtype=np.float32)
    power = power.reshape(1, -1) if power.ndim == 1 else power
    B, F = power.shape
    nf = np.clip(np.asarray(nf, dtype=np.int64).reshape(B), 0, F)
    lens = np.maximum(np.asarray(lens, dtype=np.int64).reshape(B), 0)
    ratio, floor = np.float32(ratio), np.float32(floor)
    segs, count, pmax = [], np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.float32)
    for b in range(B):
        p = power[b, :nf[b]]
        if not np.isfinite(p).all():
            segs.append(None)
            count[b], pmax[b] = -1, np.float32(np.nan)
            continue
        out = []
        if len(p):
            key = np.array([_order_keys(p).max()], dtype=np.int32)
            pmax[b] = _order_keys(key.view(np.float32)).view(np.float32)[0]
            with np.errstate(over='ignore', under='ignore'):
                thr = np.maximum(np.float32(pmax[b] * ratio), floor)
            flag = np.concatenate([[0], (p > thr).astype(np.int8), [0]])
            flips = np.flatnonzero(np.diff(flag))          # starts and ends of the raw runs, in turn
            closed = []
            for a, e in zip(flips[0::2].tolist(), flips[1::2].tolist()):
                if closed and a - closed[-1][1] < min_gap:
                    closed[-1][1] = e
                else:
                    closed.append([a, e])
            for a, e in closed:
                if e - a < min_run:
                    continue
                s0, s1 = max(0, (a - pad) * hop), min(int(lens[b]), (e - 1 + pad) * hop + win)
                if out and s0 <= out[-1][1]:
                    out[-1][1] = max(out[-1][1], s1)
                else:
                    out.append([s0, s1])
        segs.append(np.array(out, dtype=np.int64).reshape(-1, 2))
        count[b] = len(out)
    return segs, count, pmax


def frame_power64(x, n, win, hop, n_frames=None):
    """float64: the mean of x^2 over samples f hop .. f hop + win - 1 of ``x[:n]`` (zero past n) for f < n_frames (default
    ceil(n / hop)) - a cumulative sum of squares would cancel, so frames are summed one by one, vectorised over the frames"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)[:int(n)]
    if n_frames is None:
        n_frames = int(frame_count(len(x), hop))
    sq = np.zeros(max(0, (n_frames - 1) * hop + win), dtype=np.float64)
    m = min(len(sq), len(x))
    sq[:m] = x[:m] ** 2
    if n_frames == 0:
        return np.zeros(0, dtype=np.float64)
    rows = np.lib.stride_tricks.as_strided(sq, shape=(n_frames, win), strides=(hop * sq.strides[0], sq.strides[0]), writeable=False)
    return rows.sum(1) / float(win)


def _rows_and_lens(y, lens):
    is_t = hasattr(y, 'detach')
    if not is_t:
        y = np.asarray(y)
    nd = y.dim() if is_t else y.ndim
    if nd == 1:
        y = y[None, :]
    elif nd != 2:
        raise ValueError('audiogan_amd: activity takes [n] or [B, n], got %d axes' % nd)
    B, n = int(y.shape[0]), int(y.shape[1])
    ln = np.full(B, n, dtype=np.int64) if lens is None else np.clip(
        (lens.detach().cpu().numpy() if hasattr(lens, 'detach') else np.asarray(lens)).astype(np.int64).reshape(B), 0, n)
    return y, is_t, B, n, ln


def activity64(y, lens=None, sr=8000, **options):
    """the path without a GPU: the frame power in float64 numpy (``frame_power64``), rounded once to fp32, then
    ``activity_rule``.  Options and result as ``activity``."""
    y, is_t, B, n, ln = _rows_and_lens(y, lens)
    yh = y.detach().cpu().numpy() if is_t else y
    q = activity_params(sr, **options)
    nf = frame_count(ln, q['hop'])
    power = np.zeros((B, int(nf.max()) if B else 0), dtype=np.float32)
    for b in range(B):
        power[b, :nf[b]] = frame_power64(yh[b], ln[b], q['win'], q['hop']).astype(np.float32)
    return activity_rule(power, nf, ln, q['ratio'], q['floor'], q['min_gap'], q['min_run'], q['pad'], q['win'], q['hop'])[0]


def activity(y, lens=None, sr=8000, top_db=40.0, floor_db=-80.0, win_ms=25.0, hop_ms=10.0, min_gap_ms=300.0, min_run_ms=50.0,
             pad_ms=30.0, device=None, chunk=1 << 22, max_segments=256):
    """where the rows are active.  ``y`` [n] or [B, n], numpy or tensor, at ``sr`` Hz; ``lens``: samples per row (default n) ->
    a list with one int64 array [count, 2] of (start, end) samples per row, None for a row that holds a NaN or an infinity.

    A frame of ``win_ms`` every ``hop_ms`` (a row of n samples has ceil(n / hop) of them, the last ones zero-filled) is active
    when its mean power exceeds max(the row's largest / 10^(top_db / 10), 10^(floor_db / 10)).  Pauses shorter than
    ``min_gap_ms`` inside a stretch are closed, then stretches shorter than ``min_run_ms`` dropped, then ``pad_ms`` added either
    side and stretches that meet merged (``activity_rule``).  An energy gate relative to the loudest frame, as
    librosa.effects.trim / split are - not a speech detector: music or a slammed door pass it.

    On a CUDA device two launches: ``kernels.frame_power`` (one launch for a device tensor; a host source is uploaded in
    windows of ``chunk`` samples with the two starts set, which gives the bits of one launch) and
    ``kernels.activity_segments`` with K = ``max_segments``, run once more with K = the largest count when a row has more.
    Without a GPU ``activity64``: the power in float64 rounded once to fp32, the same integer rule.  The two paths can differ
    only where a frame's power lies within fp32 rounding of the threshold (or of the largest frame's, which sets it)."""
    import torch
    y, is_t, B, n, ln = _rows_and_lens(y, lens)
    if device is None:
        device = y.device if is_t and y.is_cuda else ('cuda' if torch.cuda.is_available() else 'cpu')
    device = torch.device(device)
    options = dict(top_db=top_db, floor_db=floor_db, win_ms=win_ms, hop_ms=hop_ms, min_gap_ms=min_gap_ms,
                   min_run_ms=min_run_ms, pad_ms=pad_ms)
    if device.type != 'cuda':
        return activity64(y, ln, sr, **options)
    from . import kernels as K
    q = activity_params(sr, **options)
    win, hop = q['win'], q['hop']
    nf = frame_count(ln, hop)
    F = int(nf.max()) if B else 0
    ln_t = torch.from_numpy(ln)
    power = torch.empty(B, F, dtype=torch.float32, device=device)
    if is_t and y.is_cuda:
        K.frame_power(y.float(), ln_t.to(device), win, hop, dst=power)
    else:
        per = max(1, (max(1, int(chunk)) - win) // hop + 1)          # frames whose samples fit one window
        for f0 in range(0, F, per):
            f1 = min(F, f0 + per)
            lo, hi = f0 * hop, min(n, (f1 - 1) * hop + win)
            part = y[:, lo:hi]
            part = part.float().to(device) if is_t else torch.from_numpy(np.ascontiguousarray(part, dtype=np.float32)).to(device)
            K.frame_power(part, (ln_t - lo).clamp_(0, hi - lo).to(device), win, hop, dst=power[:, f0:f1], in_start=lo, f_start=f0)
    args = (power, torch.from_numpy(nf.astype(np.int32)).to(device), ln_t.to(device), q['ratio'], q['floor'], q['min_gap'],
            q['min_run'], q['pad'], win, hop)
    seg, count, _ = K.activity_segments(*args, K=max(0, int(max_segments)))
    count = count.cpu().numpy()
    if B and int(count.max()) > seg.size(1):
        seg, _, _ = K.activity_segments(*args, K=int(count.max()))
    seg = seg.cpu().numpy()
    return [None if count[b] < 0 else seg[b, :count[b]].copy() for b in range(B)]


# ----------------------------------------------------------------------------------------------------------------------
# pitch candidates per frame: the rule of kernels.pitch_frames (ag_pitch_frames) in float64
# ----------------------------------------------------------------------------------------------------------------------
PITCH_W, PITCH_HOP, PITCH_TMIN, PITCH_TMAX, PITCH_NCCF = 256, 128, 20, 127, 112


def pitch_frame_count(n):
    """frames of a clip of n samples: those of ``kernels.melcep_frames``"""
    n = int(n)
    return (n - PITCH_W) // PITCH_HOP + 1 if n >= PITCH_W else 1


def pitch_rule64(phi, octf):
    """phi [.., 110] float64, the normalised cross-correlation at lags 19..128 -> the column (lag - 19) of the SMALLEST lag
    in 20..127 that is a local maximum (>= both neighbours) and reaches octf times the largest phi of 20..127; 0: the
    largest is not positive, or no lag qualifies"""
    mid, left, right = phi[..., 1:-1], phi[..., :-2], phi[..., 2:]
    M = mid.max(-1)
    ok = (mid >= left) & (mid >= right) & (mid >= octf * M[..., None]) & (M[..., None] > 0.0)
    return np.where(ok.any(-1), ok.argmax(-1) + 1, 0)


def pitch64(wave, lens=None, octf=0.9, center=True):
    """the rule of ``kernels.pitch_frames`` in float64 numpy: the arbiter of its tests and the path without a GPU.  ``wave``
    [L] or [B, L], ``lens``: samples per row (default L) -> (lag [B, F] int32, peak [B, F, 4], nccf [B, F, 112], nframes [B]
    int32), F the frame count of L samples; rows at or past a clip's frame count hold zeros.  Frame j is samples 128 j ..
    128 j + 383 (zeros at and past the clip's length, which is never read); ``center``: the mean of the segment's valid
    samples is subtracted from them.  phi(tau) = r / sqrt(e0 e(tau)) where that is positive, else 0, over the 256-sample
    window, tau = 19..128; the lag is ``pitch_rule64``'s; peak = phi(lag - 1), phi(lag), phi(lag + 1), e0 / 256.  ``octf`` is
    taken at its fp32 value, the one the kernel receives."""
    y, is_t, B, L, ln = _rows_and_lens(wave, lens)
    y = y.detach().cpu().numpy() if is_t else y
    octf = float(np.float32(octf))
    if not 0.0 < octf <= 1.0:
        raise ValueError('audiogan_amd: pitch64 takes octf in (0, 1], got %r' % (octf,))
    seg_len, nlag = PITCH_W + PITCH_HOP, PITCH_TMAX - PITCH_TMIN + 3
    F = pitch_frame_count(L)
    lag = np.zeros((B, F), dtype=np.int32)
    peak, nccf = np.zeros((B, F, 4)), np.zeros((B, F, PITCH_NCCF))
    nframes = np.array([pitch_frame_count(n) for n in ln], dtype=np.int32)
    t = np.arange(seg_len)
    for b in range(B):
        n, nf = int(ln[b]), int(nframes[b])
        buf = np.zeros((nf - 1) * PITCH_HOP + seg_len)
        m = min(n, len(buf))
        buf[:m] = np.asarray(y[b, :m], dtype=np.float64)
        seg = buf[np.arange(nf)[:, None] * PITCH_HOP + t[None, :]]                       # [nf, 384]
        if center:
            valid = (np.arange(nf)[:, None] * PITCH_HOP + t[None, :]) < n
            nv = valid.sum(1)
            mean = np.where(nv > 0, seg.sum(1) / np.maximum(nv, 1), 0.0)                 # (the padding adds zeros)
            seg = np.where(valid, seg - mean[:, None], 0.0)
        head = seg[:, :PITCH_W]
        e0 = (head * head).sum(1)
        phi = np.zeros((nf, nlag))
        for k in range(nlag):
            tail = seg[:, PITCH_TMIN - 1 + k:PITCH_TMIN - 1 + k + PITCH_W]
            den = e0 * (tail * tail).sum(1)
            pos = den > 0.0
            phi[pos, k] = (head * tail).sum(1)[pos] / np.sqrt(den[pos])
        col = pitch_rule64(phi, octf)
        rows = np.arange(nf)
        found = col > 0
        lag[b, :nf] = np.where(found, col + PITCH_TMIN - 1, 0)
        for d in range(3):
            peak[b, :nf, d] = np.where(found, phi[rows, np.clip(col - 1 + d, 0, nlag - 1)], 0.0)
        peak[b, :nf, 3] = e0 / float(PITCH_W)
        nccf[b, :nf, :nlag] = phi
    return lag, peak, nccf, nframes
