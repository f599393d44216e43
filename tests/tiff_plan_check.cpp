// tiff_plan_check.cpp -- r2f_tiff_header (raw2film_amd/csrc/r2f_tiff_plan.cpp) driven over frame shapes, both depths and ICC
// lengths into buffers of EXACTLY the size it asks for, under AddressSanitizer / UBSan (tests/test_output16_host.py): a write past
// the header, a shift or a conversion that overflows shows as a sanitizer report.  Checks the plan's own contract on the way.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/r2f.h"

static int fail(const char* what, int H, int W, int bits, size_t icc) {
    std::printf("FAILED: %s at H=%d W=%d bits=%d icc=%zu\n", what, H, W, bits, icc);
    return 1;
}

int main() {
    const int dims[] = {1, 2, 3, 7, 64, 257, 515, 4096, 43691, 65535, 100000};
    const size_t iccs[] = {0, 1, 2, 37, 560, 65536};
    std::vector<uint8_t> icc(65536, 0x5A);
    long cases = 0;
    for (int H : dims)
        for (int W : dims)
            for (int bits : {8, 16})
                for (size_t n_icc : iccs) {
                    r2f_tiff_plan plan;
                    size_t len = 0;
                    int rc = r2f_tiff_header(H, W, bits, n_icc ? icc.data() : nullptr, n_icc, nullptr, 0, &len, &plan);
                    const uint64_t pixels = (uint64_t)H * W * 3 * (bits / 8);
                    if (plan.file_bytes != plan.header_bytes + pixels) return fail("file size", H, W, bits, n_icc);
                    if (rc == R2F_ETOOLARGE) {
                        if (plan.file_bytes <= 0xFFFFFFFFull || len != 0) return fail("refusal", H, W, bits, n_icc);
                        ++cases;
                        continue;
                    }
                    if (rc != R2F_OK || len != plan.header_bytes || plan.header_bytes % 4) return fail("query", H, W, bits, n_icc);
                    if (plan.strips > 1 && ((uint64_t)plan.rows_per_strip * plan.row_bytes) % 2) return fail("odd strip", H, W, bits, n_icc);
                    if ((uint64_t)plan.rows_per_strip * plan.strips < (uint64_t)H || (uint64_t)plan.rows_per_strip * (plan.strips - 1) >= (uint64_t)H)
                        return fail("strips", H, W, bits, n_icc);
                    std::vector<uint8_t> buf(len);  // exactly as large as asked: ASan guards the byte behind it
                    size_t len2 = 0;
                    rc = r2f_tiff_header(H, W, bits, n_icc ? icc.data() : nullptr, n_icc, buf.data(), buf.size(), &len2, &plan);
                    if (rc != R2F_OK || len2 != len || buf[0] != 'I' || buf[2] != 42) return fail("write", H, W, bits, n_icc);
                    if (len > 1 && r2f_tiff_header(H, W, bits, n_icc ? icc.data() : nullptr, n_icc, buf.data(), len - 1, &len2, &plan) != R2F_EINVAL)
                        return fail("short buffer", H, W, bits, n_icc);
                    ++cases;
                }
    // the largest geometries an int names: H * row_bytes passes 2^64 at 16 bits and must be refused, not wrapped into a small size
    for (int bits : {8, 16}) {
        r2f_tiff_plan big;
        size_t n = 1;
        if (r2f_tiff_header(INT32_MAX, INT32_MAX, bits, nullptr, 0, nullptr, 0, &n, &big) != R2F_ETOOLARGE || n != 0 || big.file_bytes <= 0xFFFFFFFFull)
            return fail("refusal of the largest frame", INT32_MAX, INT32_MAX, bits, 0);
        if (bits == 16 && big.file_bytes != UINT64_MAX) return fail("saturated size", INT32_MAX, INT32_MAX, bits, 0);
        ++cases;
    }
    r2f_tiff_plan plan;
    size_t len;
    if (r2f_tiff_header(0, 1, 8, nullptr, 0, nullptr, 0, &len, &plan) != R2F_EINVAL || r2f_tiff_header(1, 1, 9, nullptr, 0, nullptr, 0, &len, &plan) != R2F_EINVAL ||
        r2f_tiff_header(1, 1, 8, nullptr, 5, nullptr, 0, &len, &plan) != R2F_EINVAL || r2f_tiff_header(1, 1, 8, nullptr, 0, nullptr, 0, nullptr, &plan) != R2F_EINVAL)
        return fail("bad arguments", 0, 0, 0, 0);
    std::printf("%ld cases ok\n", cases);
    return 0;
}
