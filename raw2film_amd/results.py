"""Where a rendered uint8 frame lands on the host, and who owns it then (HipProcessor._download and the streamed path):
- a pinned ring (result_buffers = n > 0): a view of one of n buffers taken in turn, valid until n more frames have come back;
- a lent pinned buffer: the caller's own array, like upstream's, without a fresh allocation -- one of up to LEASES buffers, which
  comes back when the caller's last reference to the array (or to any view of it) is gone;
- a fresh array, for a caller that holds on to more results: its pages are touched for the first time by whoever writes them (~30
  ms for 0.3 GB), so helper threads fault them in while the frame is on its way, then copy each band in as soon as it is back."""

from __future__ import annotations

import weakref
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LEASES = 3  # lent buffers of one frame size out at a time; then fresh arrays
TOUCH_PARTS = 4  # helper threads, and parts of a fresh array that are touched one by each


def touch_pages(flat, i0, i1):
    flat[i0:i1:4096] = 0  # one byte per page (NumPy releases the GIL for the strided fill)


class ResultSink:
    """One frame's way back.  `target`: the pinned buffer its device-to-host copies land in.  band_back(done, y0, y1) once the copy
    of rows y0:y1 is queued, `done` anything whose .synchronize() returns when it has landed -- an event per band if `per_band`,
    else the copy stream (an event behind every band's copy costs a streamed 100 MP frame 0.6 ms, a uint16 one 3.3); then
    finish() -> the caller's array, or abandon() on an error (with the device drained)."""

    def __init__(self, target, *, give_back=None, fresh=None, pool=None, touch=touch_pages):
        self.target = target
        self._give_back = give_back  # a lent buffer: how it comes back
        self._fresh, self._pool = fresh, pool
        self.per_band = fresh is not None  # (the fresh array is filled band by band as the bands land)
        self._done, self._copies, self._touched = None, [], []
        if fresh is not None:
            # (bytes: a page is touched once whatever the sample width; a 16-bit frame is staged as int16 holding the same bits)
            self._staged, flat = np.asarray(target).view(fresh.dtype), fresh.reshape(-1).view(np.uint8)
            self._part = -(-flat.size // TOUCH_PARTS)
            self._touched = [pool.submit(touch, flat, i, min(i + self._part, flat.size)) for i in range(0, flat.size, self._part)]

    def band_back(self, done, y0, y1):
        self._done = done
        if self._fresh is not None:
            self._copies.append(self._pool.submit(self._copy_out, done, y0, y1))

    def _copy_out(self, done, y0, y1):
        done.synchronize()  # (releases the GIL)
        row = self._fresh[0].nbytes
        # a late touch must not zero a page this copy has filled: wait for the parts that hold these rows (queued before any copy,
        # the touches are running or done by now)
        for t in self._touched[y0 * row // self._part:(y1 * row - 1) // self._part + 1]:
            t.result()
        np.copyto(self._fresh[y0:y1], self._staged[y0:y1])

    def finish(self) -> np.ndarray:
        if self._fresh is not None:
            for c in self._touched + self._copies:
                c.result()
            return self._fresh
        self._done.synchronize()
        arr = np.asarray(self.target)
        if self._give_back is not None:  # back into the pool when the caller lets go of the array
            weakref.finalize(arr, self._give_back, self.target)
        return arr

    def abandon(self):
        for c in self._touched + self._copies:
            c.cancel()
        if self._give_back is not None:
            self._give_back(self.target)


class ResultBuffers:
    """The host buffers of one processor's results of one sample type; `alloc(shape)` makes a pinned buffer of it (uint8, or the 16
    bits of a uint16 result) and `dtype` is what a fresh array is made of.  A processor keeps one of these per dtype: a lent 8-bit
    buffer never comes back as a 16-bit result, nor the other way round."""

    def __init__(self, alloc, dtype=np.uint8):
        self._alloc = alloc
        self._dtype = dtype
        self._ring, self._turn = [], 0
        self._lease_shape, self._free, self._made = None, [], 0
        self._stage, self._pool = None, None

    def lease(self, shape):
        """A buffer of `shape` to lend out, or None when LEASES of them are out.  A lent buffer comes back by `_free.append` from
        whichever thread drops the caller's last reference -- a weakref finalizer, which may run in the middle of this method, so a
        lock would have to be reentrant: instead the free list is only appended to from outside and only popped here.  A new frame
        size starts a new free list and count; the buffers of the old one are let go as they come back."""
        if shape != self._lease_shape:
            self._lease_shape, self._free, self._made = shape, [], 0
        if self._free:
            return self._free.pop()
        if self._made >= LEASES:
            return None
        self._made += 1
        return self._alloc(shape)

    def sink(self, shape, ring=0, staged=True):
        """A ring buffer (ring > 0), else a lent buffer (lease), else a fresh array staged through a pinned buffer -- or with
        staged=False None (the caller then downloads into a fresh array itself)."""
        if ring > 0:
            if len(self._ring) != ring or tuple(self._ring[0].shape) != shape:
                self._ring, self._turn = [self._alloc(shape) for _ in range(ring)], 0
            self._turn += 1
            return ResultSink(self._ring[(self._turn - 1) % ring])
        leased = self.lease(shape)
        if leased is not None:
            return ResultSink(leased, give_back=self._free.append)
        if not staged:
            return None
        if self._stage is None or tuple(self._stage.shape) != shape:
            self._stage = self._alloc(shape)
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=TOUCH_PARTS, thread_name_prefix="r2f-result")
        return ResultSink(self._stage, fresh=np.empty(shape, self._dtype), pool=self._pool)

    def borrow(self, shape):
        """(buffer, give_back) for a caller that fills a whole frame and is done with it before it returns (the TIFF export writes it
        to the file): a lent buffer and how it goes back into the pool, or -- when LEASES of them are out -- the pool's staging buffer,
        which sink() keeps for the same case, and None."""
        leased = self.lease(shape)
        if leased is not None:
            return leased, self._free.append
        if self._stage is None or tuple(self._stage.shape) != shape:
            self._stage = self._alloc(shape)
        return self._stage, None

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
        self._stage, self._pool = None, None
