// r2f_tiff_plan.cpp -- the host-side planner of the TIFF export (r2f_tiff_header, include/r2f.h): everything of a baseline TIFF 6.0
// file that is not pixel data, and where the pixel data goes.  Host-only C++ with no dependency but the C ABI header, so that it
// also builds under AddressSanitizer / UBSan (tests/test_output16_host.py).
//
// Layout (little-endian, every offset even as TIFF 6.0 asks, the pixel data 4-byte aligned):
//   0   "II" 42, offset of the IFD (8)
//   8   the IFD: entry count, 12-byte entries in ascending tag order, next-IFD offset 0
//   ..  BitsPerSample's three SHORTs, the StripOffsets and StripByteCounts arrays (when there is more than one strip), the ICC
//       profile (tag 34675, when there is one; padded to an even length)
//   ..  the strips, one behind the other: row y of the frame starts at header_bytes + y * row_bytes
#include "../../include/r2f.h"

#include <cstring>

namespace {

constexpr uint64_t kStripTarget = 256 * 1024;  // bytes per strip aimed at: a strip is what a reader decodes at once
constexpr uint64_t kClassicLimit = 0xFFFFFFFFull;  // a classic TIFF holds 32-bit offsets: the file must end at or below 4 GiB - 1

struct Writer {
    uint8_t* buf;
    size_t at;
    void u16(uint32_t v) {
        if (buf) buf[at] = (uint8_t)(v & 0xFF), buf[at + 1] = (uint8_t)((v >> 8) & 0xFF);
        at += 2;
    }
    void u32(uint64_t v) {
        if (buf)
            for (int i = 0; i < 4; ++i) buf[at + i] = (uint8_t)((v >> (8 * i)) & 0xFF);
        at += 4;
    }
    // one IFD entry whose value fits its four value bytes (a SHORT or a LONG) or lives at `value` (an offset)
    void entry(uint32_t tag, uint32_t type, uint64_t count, uint64_t value, bool short_inline = false) {
        u16(tag), u16(type), u32(count);
        if (short_inline)
            u16((uint32_t)value), u16(0);
        else
            u32(value);
    }
};

enum { kShort = 3, kLong = 4, kUndefined = 7 };

}  // namespace

extern "C" int r2f_tiff_header(int H, int W, int bits, const uint8_t* icc, size_t icc_len, uint8_t* buf, size_t cap, size_t* len,
                               r2f_tiff_plan* plan) {
    if (len) *len = 0;
    if (plan) memset(plan, 0, sizeof *plan);
    if (!len || !plan || H <= 0 || W <= 0 || (bits != 8 && bits != 16) || (icc_len && !icc) || icc_len > kClassicLimit) return R2F_EINVAL;
    const uint64_t row_bytes = (uint64_t)W * 3 * (uint64_t)(bits / 8);
    uint64_t rps = kStripTarget / row_bytes;
    if (rps < 1) rps = 1;
    if (rps > (uint64_t)H) rps = (uint64_t)H;
    // an 8-bit row of an odd width is an odd number of bytes: an even number of rows per strip keeps every strip offset on a word
    if ((row_bytes & 1) && (rps & 1) && rps < (uint64_t)H) ++rps;
    const uint64_t strips = ((uint64_t)H + rps - 1) / rps;
    const uint64_t n_entries = 11 + (icc_len ? 1 : 0);
    const uint64_t ifd_end = 8 + 2 + 12 * n_entries + 4;
    const uint64_t bps_off = ifd_end;                                   // 3 SHORTs
    const uint64_t offs_off = (bps_off + 6 + 3) / 4 * 4;                // the LONG arrays 4-byte aligned
    const uint64_t counts_off = offs_off + (strips > 1 ? 4 * strips : 0);
    const uint64_t icc_off = counts_off + (strips > 1 ? 4 * strips : 0);
    const uint64_t data_off = (icc_off + (uint64_t)icc_len + 3) / 4 * 4;
    // row_bytes < 2^34 and H < 2^31: their product can pass 2^64, so it must not wrap before it is compared (strips <= H: 4 * strips cannot)
    const bool wraps = row_bytes > (UINT64_MAX - data_off) / (uint64_t)H;
    const uint64_t file_bytes = wraps ? UINT64_MAX : data_off + row_bytes * (uint64_t)H;  // (saturated: refused below either way)
    plan->header_bytes = data_off;
    plan->file_bytes = file_bytes;
    plan->row_bytes = row_bytes;
    plan->rows_per_strip = (uint32_t)rps;
    plan->strips = (uint32_t)strips;
    if (file_bytes > kClassicLimit) return R2F_ETOOLARGE;  // (plan->file_bytes names the size)
    *len = (size_t)data_off;
    if (!buf) return R2F_OK;  // a query: the sizes alone
    if (cap < data_off) return R2F_EINVAL;
    memset(buf, 0, (size_t)data_off);
    const uint64_t last_rows = (uint64_t)H - (strips - 1) * rps;
    Writer w{buf, 0};
    w.u16(0x4949), w.u16(42), w.u32(8);
    w.u16((uint32_t)n_entries);
    w.entry(256, kLong, 1, (uint64_t)W);                      // ImageWidth
    w.entry(257, kLong, 1, (uint64_t)H);                      // ImageLength
    w.entry(258, kShort, 3, bps_off);                         // BitsPerSample -> 3 SHORTs
    w.entry(259, kShort, 1, 1, true);                         // Compression: none
    w.entry(262, kShort, 1, 2, true);                         // PhotometricInterpretation: RGB
    w.entry(273, kLong, strips, strips > 1 ? offs_off : data_off);  // StripOffsets
    w.entry(274, kShort, 1, 1, true);                         // Orientation: row 0 top, column 0 left
    w.entry(277, kShort, 1, 3, true);                         // SamplesPerPixel
    w.entry(278, kLong, 1, rps);                              // RowsPerStrip
    w.entry(279, kLong, strips, strips > 1 ? counts_off : row_bytes * last_rows);  // StripByteCounts
    w.entry(284, kShort, 1, 1, true);                         // PlanarConfiguration: chunky
    if (icc_len) w.entry(34675, kUndefined, (uint64_t)icc_len, icc_off);  // InterColorProfile
    w.u32(0);  // no further IFD
    w.at = (size_t)bps_off;
    for (int c = 0; c < 3; ++c) w.u16((uint32_t)bits);
    if (strips > 1) {
        w.at = (size_t)offs_off;
        for (uint64_t s = 0; s < strips; ++s) w.u32(data_off + s * rps * row_bytes);
        w.at = (size_t)counts_off;
        for (uint64_t s = 0; s < strips; ++s) w.u32(row_bytes * (s + 1 == strips ? last_rows : rps));
    }
    if (icc_len) memcpy(buf + icc_off, icc, icc_len);
    return R2F_OK;
}
