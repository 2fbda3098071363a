"""Minimal WAV I/O (PCM 8/16/24/32-bit and float32) so that the path does not depend on soundfile, which the reference
uses at infer.py:790 (sf.read) and :912 (sf.write PCM_16).  soundfile is used when it is installed."""
import struct
import wave

import numpy as np


def read_audio(path: str):
    """-> (float64 array [N] or [N, channels] in [-1,1), sample_rate), like soundfile.read."""
    try:
        import soundfile as sf  # noqa: WPS433
        return sf.read(path)
    except ImportError:
        pass
    try:
        with wave.open(path, "rb") as w:
            nch, width, sr, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
            raw = w.readframes(n)
    except wave.Error:
        return _read_wav_float(path)
    if width == 1:
        a = (np.frombuffer(raw, dtype=np.uint8).astype(np.float64) - 128.0) / 128.0
    elif width == 2:
        a = np.frombuffer(raw, dtype="<i2").astype(np.float64) / 32768.0
    elif width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v & 0x800000, v - 0x1000000, v)
        a = v.astype(np.float64) / 8388608.0
    elif width == 4:
        a = np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0
    else:
        raise ValueError(f"unsupported sample width {width}")
    if nch > 1:
        a = a.reshape(-1, nch)
    return a, sr


def _read_wav_float(path):
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file (compressed prompts need soundfile)")
    pos, fmt, payload = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = struct.unpack("<HHIIHH", body[:16])
        elif cid == b"data":
            payload = body
        pos += 8 + size + (size & 1)
    if fmt is None or payload is None or fmt[0] != 3 or fmt[5] != 32:
        raise ValueError(f"{path}: unsupported WAV encoding")
    a = np.frombuffer(payload, dtype="<f4").astype(np.float64)
    if fmt[1] > 1:
        a = a.reshape(-1, fmt[1])
    return a, fmt[2]


def write_pcm16(path: str, samples: np.ndarray, sample_rate: int):
    """samples int16 [N] or [N, channels] -> RIFF PCM_16 (what sf.write(..., subtype='PCM_16') produces)."""
    s = np.ascontiguousarray(samples, dtype="<i2")
    nch = 1 if s.ndim == 1 else s.shape[1]
    with wave.open(path, "wb") as w:
        w.setnchannels(nch)
        w.setsampwidth(2)
        w.setframerate(int(sample_rate))
        w.writeframes(s.tobytes())


WAV_FORMATS = {"pcm16": (1, "<i2"), "f32": (3, "<f4"), "alaw": (6, "u1"), "mulaw": (7, "u1")}   # encoding -> (format tag, sample type)


def write_wav(path: str, samples: np.ndarray, sample_rate: int, encoding: str = "pcm16"):
    """Mono samples already in `encoding` (int16 / float32 / G.711 code bytes: what the PCM output back-end produces) -> a RIFF
    file with the matching format tag: 1 PCM, 3 IEEE float, 6 A-law, 7 mu-law.  The non-PCM forms carry the 18-byte fmt chunk
    and the fact chunk the format asks of them."""
    if encoding not in WAV_FORMATS:
        raise ValueError(f"write_wav: encoding {encoding!r} is none of {sorted(WAV_FORMATS)}")
    tag, kind = WAV_FORMATS[encoding]
    s = np.ascontiguousarray(samples).reshape(-1)
    if s.dtype != np.dtype(kind):
        raise ValueError(f"write_wav: {encoding} samples are {np.dtype(kind)} (got {s.dtype})")
    data = s.astype(kind, copy=False).tobytes()
    size = np.dtype(kind).itemsize
    fmt = struct.pack("<HHIIHH", tag, 1, int(sample_rate), int(sample_rate) * size, size, 8 * size)
    if tag == 1:
        chunks = b"fmt " + struct.pack("<I", 16) + fmt
    else:
        chunks = b"fmt " + struct.pack("<I", 18) + fmt + struct.pack("<H", 0) + b"fact" + struct.pack("<II", 4, s.size)
    chunks += b"data" + struct.pack("<I", len(data)) + data + (b"\x00" if len(data) & 1 else b"")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)
