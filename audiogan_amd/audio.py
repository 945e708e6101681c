"""Audio out: what the reference's summaries write with ``librosa.output.write_wav(wav_file, sample, sr=8000)``
(audiogan.py:655-667) - a mono WAV file of 32-bit IEEE floats (format tag 3) - with the standard library only."""
import struct

import numpy as np

WAVE_FORMAT_IEEE_FLOAT = 3


def write_wav(path, samples, sr=8000):
    """write ``samples`` (1-D, any float array or tensor) to ``path`` as a mono 32-bit float WAV at ``sr`` Hz"""
    if hasattr(samples, 'detach'):
        samples = samples.detach().cpu().numpy()
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
