"""Guarded destinations for the extent tests: does a call write the rows and bytes it was given, and nothing else?

An Arena is ONE flat allocation filled with a canary; the destination a test hands to an entry point is a view placed at a
chosen element offset inside it, with a guard in front of it and one behind it.  After the call `check(written)` asserts that
every element the call was not entitled to write still holds the canary, bit for bit, and that no element it was entitled to
write still does (a missed remainder column is the same class of bug as an overrun).

Canaries no kernel of this library can produce:
  * float32: a quiet NaN with the payload 0x5CA1E (bits 0x7FC5CA1E), built from its bit pattern and compared through int32 views,
    never as a float (NaN != NaN).  Display values lie in [0, 1], densities are finite, S3 replaces a NaN; a NaN a kernel computed
    would carry the default payload.
  * integer types: every byte 0xA5.  Bin counts of frames of a few hundred thousand pixels never reach 0xA5A5A5A5.  A uint8 image
    CAN hold 0xA5 = 165 where the pixel really is 165: `check(..., expected=)` takes the values the caller compares the output
    with anyway, and an entitled element that holds the canary counts as unwritten only where the expected value is not the canary.

The guards: each holds at least two full tile heights of the tallest kernel over the frame width plus 4096 elements, so an
overshoot of a tile row -- the worst a kernel of this code base can plausibly do -- stays inside memory the test owns: a finding is
a failed assertion, never a GPU fault.  This is a condition derived from the tile constants, not a measurement.

Plain module, no fixtures; works on CPU tensors too (tests/test_arena_host.py proves that it bites).
"""

from __future__ import annotations

import numpy as np
import torch

# Rows of the tallest tile any kernel works on: the grain / tail tile is kTailQ * kTailBY = 2 * 32 = 64 rows (R2F_TAIL_BY, R2F_TAIL_Q
# in raw2film_amd/csrc/r2f_launch.h) and the largest direct-stencil variant of kStencilVariants (r2f_kernels.hip) is 128 x 64.
TALLEST_TILE_ROWS = 64
GUARD_SLACK = 4096

CANARY_F32_BITS = 0x7FC5CA1E  # quiet NaN, payload 0x5CA1E
CANARY_BYTE = 0xA5

_INT_VIEW = {torch.float32: torch.int32, torch.int32: torch.int32, torch.uint8: torch.uint8, torch.int16: torch.int16,
             torch.int64: torch.int64}


def guard_elems(W: int, channels: int = 3) -> int:
    """Elements of one guard: two tile heights of the tallest kernel over the frame width, plus slack; a multiple of 16 so that the
    view behind it keeps the allocation's alignment."""
    n = 2 * TALLEST_TILE_ROWS * int(W) * int(channels) + GUARD_SLACK
    return (n + 15) // 16 * 16


def canary_value(dtype) -> int:
    """The canary as the integer the dtype's integer view holds."""
    if dtype == torch.float32:
        return int(np.array([CANARY_F32_BITS], dtype=np.uint32).view(np.int32)[0])
    size = torch.empty((), dtype=dtype).element_size()
    return int(np.frombuffer(bytes([CANARY_BYTE]) * size, dtype={1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[size])[0])


class Arena:
    """One flat canary-filled allocation and a view inside it.  `view` is what the entry point gets; `names` label the view's
    dimensions in messages (("plane", "row", "column") for planes)."""

    def __init__(self, dtype, shape, strides, *, guard: int, misalign: int = 0, device="cpu", names=None):
        shape, strides = tuple(int(s) for s in shape), tuple(int(s) for s in strides)
        assert len(shape) == len(strides) and guard % 16 == 0 and misalign >= 0
        assert guard >= 2 * TALLEST_TILE_ROWS + GUARD_SLACK, "a guard is two tile heights plus slack (guard_elems)"
        self.dtype, self.shape, self.strides = dtype, shape, strides
        self.start = guard + misalign
        span = 1 + sum((n - 1) * s for n, s in zip(shape, strides)) if all(shape) else 0
        self.total = self.start + span + guard + 16
        self.names = tuple(names) if names else tuple(f"dim{i}" for i in range(len(shape)))
        self._ibits = _INT_VIEW[dtype]
        self.canary = canary_value(dtype)
        self.buf = torch.empty(self.total, dtype=dtype, device=device)
        self.buf.view(self._ibits).fill_(self.canary)
        self.view = torch.as_strided(self.buf, shape, strides, self.start)
        # flat offset of every element of the view (host side: the geometry, not the data)
        self._index = torch.as_strided(torch.arange(self.total, dtype=torch.int64), shape, strides, self.start)

    # ------------------------------------------------------------------ constructors
    @classmethod
    def planes(cls, rows_alloc: int, W: int, *, pad: int = 0, misalign: int = 0, device="cpu"):
        """(3, rows_alloc, W) float32 planes, plane stride rows_alloc * W + pad floats, `misalign` floats past a 16-byte boundary:
        contiguous when pad = 0, otherwise what a row slice t[:, a:b, :] of a taller tensor looks like (HipContext.planes takes both)."""
        assert pad in (0, 1, 4) and misalign in (0, 1)
        return cls(torch.float32, (3, rows_alloc, W), (rows_alloc * W + pad, W, 1), guard=guard_elems(W), misalign=misalign,
                   device=device, names=("plane", "row", "column"))

    @classmethod
    def hwc(cls, rows_alloc: int, W: int, dtype=torch.float32, *, misalign: int = 0, channels: int = 3, device="cpu"):
        """(rows_alloc, W, channels) interleaved output, `misalign` ELEMENTS past a 16-byte boundary (1 byte for uint8)."""
        return cls(dtype, (rows_alloc, W, channels), (W * channels, channels, 1), guard=guard_elems(W, channels), misalign=misalign,
                   device=device, names=("row", "column", "channel"))

    @classmethod
    def flat(cls, nbytes: int, *, misalign: int = 0, device="cpu"):
        """`nbytes` bytes (a workspace, a JPEG output): a uint8 view; reinterpret it with .view.view(dtype) when the offset allows."""
        return cls.flat_of(torch.uint8, nbytes, misalign=misalign, device=device)

    @classmethod
    def flat_of(cls, dtype, n: int, *, misalign: int = 0, device="cpu"):
        """n elements of `dtype` (histogram counts, burn sums, the JPEG length word)."""
        return cls(dtype, (int(n),), (1,), guard=guard_elems(64, 1), misalign=misalign, device=device, names=("offset",))

    @classmethod
    def holding(cls, t, *, misalign: int = 0, pad: int = 0, device=None):
        """An arena whose view is a copy of the contiguous tensor `t` (a source buffer: check it with unchanged()).  pad: extra
        elements between the slices of the first dimension."""
        t = t.contiguous()
        strides = list(t.stride())
        if pad and t.dim() > 1:
            strides[0] += pad
        interleaved = t.dim() == 3 and t.shape[-1] <= 4  # (rows, W, channels); otherwise the last dimension is a row
        row = int(t.shape[-1]) * (int(t.shape[-2]) if interleaved else 1)
        a = cls(t.dtype, t.shape, strides, guard=guard_elems(max(row, 1), 1 if interleaved or t.dim() < 3 else 3),
                misalign=misalign, device=device if device is not None else t.device)
        a.view.copy_(t)
        a._snapshot = a.buf.clone()
        return a

    # ------------------------------------------------------------------ masks
    def rows_mask(self, r0: int, r1: int, planes=None):
        """Boolean mask of the view: rows [r0, r1) of the given planes (all by default) of a planes view, or of an interleaved one."""
        m = torch.zeros(self.shape, dtype=torch.bool)
        if self.names[0] == "plane":
            for p in (range(self.shape[0]) if planes is None else planes):
                m[p, r0:r1] = True
        else:
            assert planes is None
            m[r0:r1] = True
        return m

    def _mask(self, written):
        if written is None or (isinstance(written, (list, tuple)) and len(written) == 0):
            return torch.zeros(self.shape, dtype=torch.bool)
        if isinstance(written, torch.Tensor):
            assert tuple(written.shape) == self.shape and written.dtype == torch.bool
            return written.cpu()
        m = torch.zeros(self.shape, dtype=torch.bool)
        for plane, (r0, r1) in written:  # list of (plane, row range); plane None: every plane / an interleaved view
            m |= self.rows_mask(r0, r1, None if plane is None else [plane])
        return m

    # ------------------------------------------------------------------ checks
    def where(self, flat_offset: int) -> str:
        """A flat offset as coordinates relative to the view (rows < 0 or >= the view's: in front of / behind it or in a plane's pad)."""
        rel = int(flat_offset) - self.start
        if len(self.shape) == 1:
            return f"{self.names[0]} {rel}"
        coords, rem = [], rel
        if len(self.shape) == 3 and self.names[0] == "plane":
            p = min(max(rem // self.strides[0], 0), self.shape[0] - 1)
            coords.append(p)
            rem -= p * self.strides[0]
            dims = (1, 2)
        else:
            dims = tuple(range(len(self.shape)))
        for k, d in enumerate(dims):
            if k == len(dims) - 1:
                coords.append(rem // self.strides[d])
            else:
                q = rem // self.strides[d]  # floor: a negative row for an offset in front of the view
                coords.append(q)
                rem -= q * self.strides[d]
        return " / ".join(f"{n} {c}" for n, c in zip(self.names, coords)) + f" (element {rel:+d} from the view's base)"

    def check(self, written, *, expected=None, require_written: bool = True, what: str = ""):
        """written: boolean mask of the view's shape, or a list of (plane, (row0, row1)) in the view's own row numbering, that the
        call was entitled to write.  Asserts that everything else in the allocation still holds the canary and -- unless
        require_written is off (bytes a call may but need not write) -- that nothing entitled still does.  expected: the values the
        entitled region should hold (view-shaped); an entitled element equal to the canary is then excused where the expected
        value is the canary itself (a uint8 pixel that really is 0xA5)."""
        mask = self._mask(written)
        entitled = torch.zeros(self.total, dtype=torch.bool)
        entitled[self._index[mask]] = True
        bits = self.buf.view(self._ibits).cpu()
        is_canary = bits == self.canary
        bad = (~entitled) & (~is_canary)
        if bool(bad.any()):
            off = int(torch.nonzero(bad)[0])
            raise AssertionError(f"{what}: wrote outside its rows: {int(bad.sum())} element(s), first at {self.where(off)}, "
                                 f"bits {int(bits[off]) & (2 ** (8 * bits.element_size()) - 1):#x}")
        if require_written:
            left = entitled & is_canary
            if expected is not None:
                exp = torch.as_tensor(expected).to(self.dtype).contiguous().view(self._ibits).cpu()
                assert tuple(exp.shape) == self.shape
                excuse = torch.zeros(self.total, dtype=torch.bool)
                excuse[self._index[mask & (exp == self.canary)]] = True
                left &= ~excuse
            if bool(left.any()):
                off = int(torch.nonzero(left)[0])
                raise AssertionError(f"{what}: left {int(left.sum())} element(s) of its rows unwritten, first at {self.where(off)}")

    def unchanged(self, what: str = ""):
        """A source arena (holding()): every byte, the view's and the guards', is what it was."""
        now, then = self.buf.view(self._ibits).cpu(), self._snapshot.view(self._ibits).cpu()
        diff = now != then
        if bool(diff.any()):
            off = int(torch.nonzero(diff)[0])
            raise AssertionError(f"{what}: the call changed its source: {int(diff.sum())} element(s), first at {self.where(off)}")
