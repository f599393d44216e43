"""TIFF export of a rendered frame (HipProcessor.process_tiff): baseline TIFF 6.0, little-endian, uncompressed, chunky RGB at 8
or 16 bits per sample, Orientation 1, an optional ICC profile in tag 34675.  Everything but the pixels -- the IFD, the strip tables,
the profile -- is the header r2f_tiff_header plans on the host (raw2film_amd/csrc/r2f_tiff_plan.cpp); the strips follow it one
behind the other, so row y of the frame is the `row_bytes` bytes at `header_bytes + y * row_bytes` and a frame that arrives in row
bands can be written band by band behind a header that is complete before the first pixel exists."""

from __future__ import annotations

import ctypes as C
import io
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib


def check_icc(icc_profile) -> bytes:
    if not isinstance(icc_profile, (bytes, bytearray, memoryview)):
        raise ValueError(f"icc_profile must be bytes, got {type(icc_profile).__name__}")
    return bytes(icc_profile)


def header(H: int, W: int, bits: int, icc_profile: bytes = b""):
    """(the file's header as bytes, its r2f_tiff_plan) for an H x W frame of `bits` bits per sample.  No GPU.  A file past a
    classic TIFF's 4 GiB is refused with a ValueError that names its size."""
    lib = _lib.load()
    icc = check_icc(icc_profile)
    plan, n = _lib.TiffPlan(), C.c_size_t()
    icc_buf = (C.c_uint8 * len(icc)).from_buffer_copy(icc) if icc else None
    rc = lib.r2f_tiff_header(int(H), int(W), int(bits), icc_buf, len(icc), None, 0, C.byref(n), C.byref(plan))
    if rc == _lib.ETOOLARGE:
        raise ValueError(f"a {int(H)} x {int(W)} frame at {int(bits)} bits is a TIFF file of {int(plan.file_bytes)} bytes: a classic "
                         "TIFF holds less than 4 GiB (4294967296 bytes)")
    if rc != 0:
        raise ValueError(f"r2f_tiff_header: a non-empty frame at 8 or 16 bits is required, got {H} x {W} at {bits} bits")
    buf = (C.c_uint8 * n.value)()
    rc = lib.r2f_tiff_header(int(H), int(W), int(bits), icc_buf, len(icc), buf, n.value, C.byref(n), C.byref(plan))
    if rc != 0:
        raise RuntimeError(f"r2f_tiff_header failed with code {rc}")
    return bytes(buf), plan


def _pixels(array) -> np.ndarray:
    if not (isinstance(array, np.ndarray) and array.ndim == 3 and array.shape[2] == 3 and array.dtype in (np.uint8, np.uint16)):
        raise ValueError("a TIFF frame must be a uint8 or uint16 (H, W, 3) array")
    return np.ascontiguousarray(array.astype(array.dtype.newbyteorder("<"), copy=False))


def encode(array, icc_profile: bytes = b"") -> bytes:
    """The one-piece file of a uint8 / uint16 (H, W, 3) host array."""
    px = _pixels(array)
    head, _ = header(px.shape[0], px.shape[1], 8 * px.dtype.itemsize, icc_profile)
    return head + px.tobytes()


def deliver(array, icc_profile, file):
    """The file of `array` as bytes (file=None), or written into `file` (a path or a binary file object) -> its byte count."""
    px = _pixels(array)
    head, plan = header(px.shape[0], px.shape[1], 8 * px.dtype.itemsize, icc_profile)
    if file is None:
        return head + px.tobytes()
    if isinstance(file, (str, bytes)) or hasattr(file, "__fspath__"):
        with open(file, "wb") as f:
            f.write(head)
            f.write(px.data)
    else:
        file.write(head)
        file.write(px.data)
    return int(plan.file_bytes)


class TiffBandSink:
    """The way back of a frame that streams through the pipeline in row bands, into a TIFF file (the interface of
    results.ResultSink, which HipProcessor._run_bands fills): the header goes into the file first, then every band's rows as soon
    as their copy into `target` -- a pinned (H, W, 3) buffer -- has landed, in row order, from one writer thread, while later bands
    are still being rendered.  finish() -> the byte count (a file was given) or the file's bytes."""

    per_band = True  # an event behind every band's copy: the writer waits for exactly that band

    def __init__(self, target, head: bytes, plan, file, give_back=None):
        self.target, self._give_back = target, give_back
        self._rows = np.asarray(target)
        self._bytes = int(plan.file_bytes)
        self._own = isinstance(file, (str, bytes)) or hasattr(file, "__fspath__")
        self._memory = file is None
        self._f = io.BytesIO() if file is None else open(file, "wb") if self._own else file
        self._f.write(head)
        self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="r2f-tiff")
        self._writes = []

    def _write(self, done, y0, y1):
        done.synchronize()  # (releases the GIL)
        self._f.write(self._rows[y0:y1].data)

    def band_back(self, done, y0, y1):
        self._writes.append(self._pool.submit(self._write, done, y0, y1))

    def _close(self):
        self._pool.shutdown(wait=True)
        if self._own:
            self._f.close()
        if self._give_back is not None:
            self._give_back(self.target)
            self._give_back = None

    def finish(self):
        try:
            for w in self._writes:
                w.result()
            data = self._f.getvalue() if self._memory else None
        finally:
            self._close()
        return data if self._memory else self._bytes

    def abandon(self):
        for w in self._writes:
            w.cancel()
        self._close()
