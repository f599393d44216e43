"""The file formats of HipProcessor._export, which process_jpeg / process_tiff and their process_preloaded_* twins share.  A format:
- `name`: "jpeg" / "tiff", for the calls' messages (process_<name>, process_preloaded_<name>);
- `early`: its own reasons not to stream, known from its options alone (None where one does not apply);
- `bits`: the sample width its band path renders at;
- sink(proc, depth, out, bounds, file) -> (sink, band_done) as HipProcessor._stream takes them: where the finished rows of the
  streamed frame's device result `out` go;
- whole(proc, out, file): the file of a frame rendered in one piece -> its bytes, or with `file` their count."""

from __future__ import annotations

from . import tiff
from .jpeg_stream import JpegBandSink, JpegStaging, deliver


class JpegExport:
    """`o`: the call's checked options (jpeg_options.checked_options; optimize and progressive never stream: o.early)."""
    name, bits = "jpeg", 8  # (a JPEG is 8 bits per sample whatever `output_bits` the caller's settings carry)

    def __init__(self, o):
        self.o, self.early = o, o.early

    def sink(self, proc, depth, out_u8, bounds, file):
        """No pixels come down: each band's finished MCU rows are encoded behind its tail, the file's final bytes follow (jpeg_stream.py)."""
        if proc._jpeg_staging is None:
            proc._jpeg_staging = JpegStaging(proc._torch, proc.device)
        o, x = self.o, self.o.extras
        sink = JpegBandSink(proc._jpeg_staging, proc.ctx, out_u8, o.quality, bounds, proc._copy_streams()[1], file, o.subsampling,
                            segments=x.segments(o.exif), restart=x.restart(int(out_u8.shape[1]), o.subsampling), density=x.density)
        return sink, sink.band

    def whole(self, proc, out_u8, file):
        return deliver(proc._encode_device(out_u8, self.o), file)


class TiffExport:
    """`bits`: 8 or 16 per sample; `icc`: the profile's bytes (tiff.check_icc)."""
    name, early = "tiff", ()

    def __init__(self, bits, icc):
        self.bits, self.icc = bits, icc

    def sink(self, proc, depth, out, bounds, file):
        """The header first, then every band's rows into the file behind their download (tiff.TiffBandSink)."""
        H, W = int(out.shape[0]), int(out.shape[1])
        head, plan = tiff.header(H, W, depth.bits, self.icc)  # (refuses a file past 4 GiB before any band runs)
        target, give_back = depth.pool.borrow((H, W, 3))
        return tiff.TiffBandSink(target, head, plan, file, give_back), None

    def whole(self, proc, out, file):
        return tiff.deliver(proc._download(out), self.icc, file)
