"""Packed 24-bit PCM (BPMX_DT_I24) on the host.

numpy has no int24, and ``scipy.io.wavfile.read`` expands every 3-byte sample
of a 24-bit WAV into an ``int32`` holding ``v << 8``.  ``Pcm24`` keeps the
bytes as they lie in the file, so 3 bytes per sample are uploaded instead of
4; the library treats them as exactly that int32 array (include/bpmx.h).
"""
from __future__ import annotations

import struct

import numpy as np

SAMPLE_FORMAT = "i24"                  # Detector.run(..., sample_format=...)

_PCM_GUID_TAIL = b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"   # KSDATAFORMAT_SUBTYPE_PCM after its tag


class _Format:
    """Stands where an array has its dtype: groups and compares as a format of its own."""
    str = "<i3"
    name = "int24"
    itemsize = 3

    def __eq__(self, other):
        return isinstance(other, _Format)

    def __ne__(self, other):
        return not isinstance(other, _Format)

    def __hash__(self):
        return hash("<i3")

    def __repr__(self):
        return "pcm24"


class Pcm24:
    """One recording of packed 24-bit samples: ``data`` is a contiguous uint8
    array of ``3 * frames * channels`` bytes (little-endian, two's complement,
    frames interleaved)."""
    dtype = _Format()

    def __init__(self, data: np.ndarray, channels: int = 1):
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        channels = int(channels)
        if channels < 1 or data.size % (3 * channels):
            raise ValueError("packed 24-bit PCM needs a whole number of 3-byte frames")
        self.data = data
        self.channels = channels

    @property
    def shape(self):
        n = self.data.size // (3 * self.channels)
        return (n,) if self.channels == 1 else (n, self.channels)

    @property
    def ndim(self) -> int:
        return 1 if self.channels == 1 else 2

    def __len__(self) -> int:
        return self.shape[0]

    def to_int32(self) -> np.ndarray:
        """The array scipy.io.wavfile.read gives for the same file: ``v << 8`` as int32."""
        b = self.data.reshape(-1, 3)
        a = np.zeros((b.shape[0], 4), np.uint8)
        a[:, 1:] = b
        return a.view("<i4").reshape(self.shape).astype(np.int32, copy=False)

    @classmethod
    def from_int32(cls, a: np.ndarray) -> "Pcm24":
        """From an int32 array (frames,) or (frames, channels) whose low bytes are zero."""
        a = np.asarray(a)
        if a.dtype != np.int32 or a.ndim not in (1, 2):
            raise ValueError("from_int32 needs an int32 array of one or two dimensions")
        if np.any(a & 0xFF):
            raise ValueError("from_int32: samples with non-zero low bytes are not 24-bit")
        b = np.ascontiguousarray(a).astype("<i4", copy=False).reshape(-1).view(np.uint8).reshape(-1, 4)
        return cls(b[:, 1:].copy(), 1 if a.ndim == 1 else a.shape[1])


def _scipy_read(path):
    import warnings

    from scipy.io import wavfile
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return wavfile.read(path)


def _parse(raw: bytes):
    """(fs, channels, data offset, data size) of a plain 24-bit PCM RIFF file, else None."""
    if len(raw) < 12 or raw[:4] != b"RIFF" or raw[8:12] != b"WAVE":
        return None
    pos, fmt = 12, None
    while pos + 8 <= len(raw):
        cid, size = raw[pos:pos + 4], struct.unpack_from("<I", raw, pos + 4)[0]
        body = pos + 8
        if cid == b"fmt ":
            if fmt is not None or size < 16 or body + size > len(raw):
                return None
            tag, ch, fs, _, align, bits = struct.unpack_from("<HHIIHH", raw, body)
            if tag == 0xFFFE:
                if size < 40:
                    return None
                cb, valid = struct.unpack_from("<HH", raw, body + 16)
                if cb < 22 or valid != 24 or raw[body + 24:body + 26] != b"\x01\x00" or \
                        raw[body + 26:body + 40] != _PCM_GUID_TAIL:
                    return None
            elif tag != 1:
                return None
            if bits != 24 or ch < 1 or align != 3 * ch or fs < 1:
                return None
            fmt = (fs, ch)
        elif cid == b"data":
            if fmt is None or body + size > len(raw) or size % (3 * fmt[1]):
                return None
            return fmt[0], fmt[1], body, size
        pos = body + size + (size & 1)
    return None


def read_wav(path):
    """``(fs, Pcm24)`` for a plain 24-bit PCM WAV (format tag 1, or the
    extensible tag with the PCM sub-format), its samples not expanded.  Any
    other file, and any this parser is not sure about, is read by
    ``scipy.io.wavfile.read`` and returned as that returns it."""
    try:
        with open(path, "rb") as fh:
            raw = fh.read()
        got = _parse(raw)
    except (OSError, struct.error):
        got = None
    if got is None:
        return _scipy_read(path)
    fs, ch, off, size = got
    return fs, Pcm24(np.frombuffer(raw, np.uint8, size, off).copy(), ch)
