"""The streamed JPEG export (HipProcessor.process_jpeg / process_preloaded_jpeg with stream=True): as the band loop finishes a
band's tail, the MCU rows that are now complete are encoded row-wise on the device (HipContext.jpeg_rows), and the bytes of the
file that became final go down and into the file while later bands are still on their way up.
- jpeg_row_steps: which rows the encoder takes after each band -- a pure function of the band bounds;
- JpegStaging: what a processor keeps between exports: a ring of pinned chunks, pinned length words, a copy stream, two threads;
- JpegBandSink: one export.  The launching thread only queues work: after band b's encode, a snapshot of the final-bytes word
  goes down into pinned memory on the download stream; the fetch thread waits for it and queues the copies of the new bytes, a
  chunk at a time, into free ring slots; the write thread waits for each copy, writes the chunk and frees its slot.  (One writer:
  four threads writing a path's chunks at their offsets measured no faster, tools/jpeg_stream_probe.py.)"""

from __future__ import annotations

import io
import os
import queue
from concurrent.futures import ThreadPoolExecutor

CHUNK = 8 << 20  # bytes per slot of the pinned ring (a 101 MP file of ~130 MB at quality 100 arrives in ~8 MB per band)
SLOTS = 4


def jpeg_row_steps(bounds, H, mcu_height=16):
    """Per band of `bounds` (plan_bands': 0 = bounds[0] < ... < bounds[-1] = H): the rows (y0, y1) the encoder takes once that
    band's tail is done, or None.  Rows [0, bounds[b + 1]) exist then; the encoder takes them up to the last multiple of the MCU
    height (an MCU row reads 16 rows in 4:2:0, 8 in 4:2:2 and 4:4:4), the last band up to H.  The steps partition [0, H) in
    order."""
    steps, done = [], 0
    for b in range(len(bounds) - 1):
        y1 = H if bounds[b + 1] >= H else bounds[b + 1] // mcu_height * mcu_height
        steps.append((done, y1) if y1 > done else None)
        done = max(done, y1)
    return steps


class JpegStaging:
    """A processor's host side of the streamed export, made on its first one and kept (HipProcessor.close() frees it): nothing in
    it is allocated inside the band loop."""

    def __init__(self, torch, device):
        self._torch, self.device = torch, device
        self.ring = torch.empty((SLOTS, CHUNK), dtype=torch.uint8, pin_memory=True)
        self.ring_np = self.ring.numpy()
        self.free = queue.SimpleQueue()
        for i in range(SLOTS):
            self.free.put(i)
        self.lens = None  # pinned int64: the final-bytes word after each band's encode
        self.stream = torch.cuda.Stream(device=device)  # the file's bytes go down on this one
        self.fetcher = ThreadPoolExecutor(max_workers=1, thread_name_prefix="r2f-jpeg-fetch", initializer=torch.cuda.set_device,
                                          initargs=(device,))
        self.writer = ThreadPoolExecutor(max_workers=1, thread_name_prefix="r2f-jpeg-write")

    def lengths(self, n):
        if self.lens is None or self.lens.numel() < n:  # (grows only: 64 covers every band count plan_bands makes by default)
            self.lens = self._torch.empty(max(n, 64), dtype=self._torch.int64, pin_memory=True)
        return self.lens

    def close(self):
        self.fetcher.shutdown(wait=True)
        self.writer.shutdown(wait=True)
        self.ring = self.ring_np = self.lens = None


def app1_segment(exif: bytes) -> bytes:
    """The APP1 segment Pillow writes for `exif` (b"" for none): FF E1, the length + 2 (big-endian), the bytes.  It goes right after
    the file's first 20 bytes (SOI + APP0)."""
    return b"\xff\xe1" + (len(exif) + 2).to_bytes(2, "big") + exif if exif else b""


MARKER_MAX = 65533  # a marker segment's payload (Pillow's MAX_BYTES_IN_MARKER)
XMP_NAMESPACE = b"http://ns.adobe.com/xap/1.0/\x00"
ICC_OVERHEAD = 14   # b"ICC_PROFILE\0", the chunk's number from 1, the chunk count


def _segment(marker: int, payload: bytes) -> bytes:
    return bytes((0xFF, marker)) + (len(payload) + 2).to_bytes(2, "big") + payload


def metadata_segments(exif: bytes = b"", xmp: bytes = b"", icc_profile: bytes = b"", comment: bytes = b"") -> bytes:
    """Every variable-length segment of an export in the order Pillow writes them, to go right after the file's first 20 bytes
    (SOI + APP0): APP1 Exif, APP1 XMP (its namespace first), the profile in APP2 chunks of at most 65533 - 14 bytes, COM.  Each
    empty one is left out; the lengths were checked with the options (jpeg_options._jpeg_extras)."""
    out = [app1_segment(exif)]
    if xmp:
        out.append(_segment(0xE1, XMP_NAMESPACE + xmp))
    step = MARKER_MAX - ICC_OVERHEAD
    chunks = [icc_profile[i:i + step] for i in range(0, len(icc_profile), step)]
    for i, chunk in enumerate(chunks):
        out.append(_segment(0xE2, b"ICC_PROFILE\0" + bytes((i + 1, len(chunks))) + chunk))
    if comment:
        out.append(_segment(0xFE, comment))
    return b"".join(out)


def open_output(file):
    """(binary file object, whether this call opened it) for a path or a file object; (BytesIO, False) for None."""
    if file is None:
        return io.BytesIO(), False
    if isinstance(file, (str, bytes, os.PathLike)):
        return open(file, "wb"), True
    if not callable(getattr(file, "write", None)):
        raise TypeError(f"file: a path or a binary file object, got {type(file).__name__}")
    return file, False


class JpegBandSink:
    """One streamed export: band(b) after band b's tail (on the launching thread), then finish() -> the file's bytes (file=None)
    or its length, or abandon() on an error with the device drained.  subsampling: 0 4:4:4, 1 4:2:2, 2 4:2:0; exif: the bytes of
    an APP1 segment the writer puts after the file's first 20 bytes (b"": none), or with `segments` every such segment ready
    made (metadata_segments); restart, density: r2f_jpeg_opts' restart_interval and (x_density, y_density)."""

    def __init__(self, staging, ctx, image_u8, quality, bounds, down, file=None, subsampling=2, exif=b"", *, segments=None,
                 restart=0, density=(0, 0)):
        torch = ctx._torch
        H, W = int(image_u8.shape[0]), int(image_u8.shape[1])
        self._torch, self._st, self._image, self._down = torch, staging, image_u8, down
        self.steps = jpeg_row_steps(bounds, H, 16 if subsampling == 2 else 8)
        # (written by the first write, ahead of every scan byte: every first chunk holds the whole header)
        self._app1 = app1_segment(exif) if segments is None else segments
        self._app1_pending = bool(self._app1)
        self._lens = staging.lengths(len(self.steps))
        self._lens_np = self._lens.numpy()
        self._file, self._own = open_output(file)
        self._return_bytes = file is None
        self._failed = False
        self._sent = 0  # bytes of the file whose copy down is queued
        self._fetches, self._writes = [], []
        self._compute = torch.cuda.current_stream(ctx.device)
        self._snap = torch.empty(len(self.steps), dtype=torch.int64, device=ctx.device)  # the word after each band's encode
        try:
            self.enc = ctx.jpeg_rows(H, W, quality, subsampling, restart, density)  # (header and carry written on the launching stream)
        except BaseException:
            self._close_file()
            raise

    def band(self, b):
        step = self.steps[b]
        if step is None:
            return
        torch = self._torch
        self.enc.rows(self._image, *step)
        self._snap[b:b + 1].copy_(self.enc.length)  # (the next band's encode overwrites the word: each band reads its own copy)
        done = self._compute.record_event()
        with torch.cuda.stream(self._down):
            self._down.wait_event(done)
            self._lens[b:b + 1].copy_(self._snap[b:b + 1], non_blocking=True)
            landed = self._down.record_event()
        self._fetches.append(self._st.fetcher.submit(self._fetch, b, landed))

    def _fetch(self, b, landed):
        landed.synchronize()
        n = int(self._lens_np[b])
        if n <= 0:
            raise RuntimeError("r2f_jpeg_rows reported a broken bound (the final-bytes word is 0)")
        torch, st = self._torch, self._st
        while self._sent < n and not self._failed:
            slot = st.free.get()  # (a slot comes back when its write is done)
            a, m = self._sent, min(n - self._sent, CHUNK)
            with torch.cuda.stream(st.stream):
                st.ring[slot, :m].copy_(self.enc.out[a:a + m], non_blocking=True)
                copied = st.stream.record_event()
            self._writes.append(st.writer.submit(self._write, slot, copied, m))
            self._sent = a + m

    def _write(self, slot, copied, m):
        try:
            copied.synchronize()
            if not self._failed:
                chunk = memoryview(self._st.ring_np[slot, :m])
                if self._app1_pending:
                    self._file.write(chunk[:20])
                    self._file.write(self._app1)
                    chunk = chunk[20:]
                    self._app1_pending = False
                self._file.write(chunk)
        except BaseException:
            self._failed = True
            raise
        finally:
            self._st.free.put(slot)

    def finish(self):
        for f in self._fetches:
            f.result()
        for w in self._writes:  # (complete: the fetches that append to it are done)
            w.result()
        if not self.enc.done:
            raise RuntimeError("the streamed export ended before the frame's last rows")
        n = self._sent + len(self._app1)
        out = self._file.getvalue() if self._return_bytes else n
        self._close_file()
        return out

    def abandon(self):
        self._failed = True  # (no further copies are queued, queued writes only hand their slots back)
        for futures in (self._fetches, self._writes):  # (the writes once every fetch that queues them is done)
            for f in futures:
                try:
                    f.result()
                except BaseException:
                    pass
        self._close_file()

    def _close_file(self):
        if self._own:
            self._file.close()
            self._own = False


def deliver(data: bytes, file):
    """A finished file: `data` itself (file=None), or written into `file` (a path or a binary file object) -> its length."""
    if file is None:
        return data
    f, own = open_output(file)
    try:
        f.write(data)
    finally:
        if own:
            f.close()
    return len(data)

