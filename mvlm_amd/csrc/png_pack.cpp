// Host side of the device PNG encoder: layout, bound, Adler-32 combination, file assembly (png_pack.h).  No device code.
#include "png_pack.h"

#include <cstring>

using namespace mvlm_png;

int mvlm_png_layout(int height, int width, Layout& out, std::string& why) {
    if (height < 1 || height > MAX_DIM || width < 1 || width > MAX_DIM) {
        why = "png: height and width must be 1..4096 (" + std::to_string(height) + " x " + std::to_string(width) + " given)";
        return 1;
    }
    out.height = height;
    out.width = width;
    out.row_bytes = 1 + 3 * size_t(width);
    out.stream_bytes = size_t(height) * out.row_bytes;
    out.n_segments = int((out.stream_bytes + SEGMENT - 1) / SEGMENT);
    out.last_bytes = out.stream_bytes - size_t(out.n_segments - 1) * SEGMENT;
    out.payload_cap = out.stream_bytes + size_t(out.n_segments) * SEG_SLACK;
    out.bound = HEAD_BYTES + out.payload_cap + TAIL_BYTES;
    return 0;
}

uint32_t mvlm_png_adler_combine(const Layout& lay, const uint32_t* ab) {
    uint64_t a = 1, b = 0;
    for (int s = 0; s < lay.n_segments; ++s) {
        const uint64_t n = s + 1 < lay.n_segments ? uint64_t(SEGMENT) : uint64_t(lay.last_bytes);
        b = (b + n % ADLER_MOD * a + ab[2 * s + 1] % ADLER_MOD) % ADLER_MOD;  // (before a moves on)
        a = (a + ab[2 * s] % ADLER_MOD) % ADLER_MOD;
    }
    return uint32_t(b << 16 | a);
}

namespace {

struct CrcTable {
    uint32_t t[8][256];
    CrcTable() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int k = 1; k < 8; ++k) t[k][i] = t[0][t[k - 1][i] & 0xFFu] ^ (t[k - 1][i] >> 8);
    }
};

void put_be32(uint8_t* p, uint32_t v) {
    p[0] = uint8_t(v >> 24);
    p[1] = uint8_t(v >> 16);
    p[2] = uint8_t(v >> 8);
    p[3] = uint8_t(v);
}

}  // namespace

uint32_t mvlm_png_crc32(uint32_t crc, const uint8_t* data, size_t n) {
    static const CrcTable tab;
    uint32_t c = ~crc;
    while (n >= 8) {  // eight bytes a step
        const uint32_t lo = c ^ (uint32_t(data[0]) | uint32_t(data[1]) << 8 | uint32_t(data[2]) << 16 | uint32_t(data[3]) << 24);
        c = tab.t[7][lo & 0xFFu] ^ tab.t[6][(lo >> 8) & 0xFFu] ^ tab.t[5][(lo >> 16) & 0xFFu] ^ tab.t[4][lo >> 24] ^
            tab.t[3][data[4]] ^ tab.t[2][data[5]] ^ tab.t[1][data[6]] ^ tab.t[0][data[7]];
        data += 8;
        n -= 8;
    }
    for (; n; --n) c = tab.t[0][(c ^ *data++) & 0xFFu] ^ (c >> 8);
    return ~c;
}

int mvlm_png_finish(uint8_t* file, size_t capacity, const Layout& lay, size_t payload_bytes, uint32_t adler, size_t* file_bytes,
                    std::string& why) {
    if (!file || !file_bytes) {
        why = "png: null pointer";
        return 1;
    }
    if (payload_bytes > lay.payload_cap || payload_bytes < size_t(lay.n_segments)) {
        why = "png: the segments' bytes (" + std::to_string(payload_bytes) + ") do not fit the layout";
        return 1;
    }
    const size_t total = HEAD_BYTES + payload_bytes + TAIL_BYTES;
    if (total > capacity) {
        why = "png: the file needs " + std::to_string(total) + " bytes, the buffer holds " + std::to_string(capacity);
        return 1;
    }
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    uint8_t* p = file;
    std::memcpy(p, sig, 8);
    put_be32(p + 8, 13);
    std::memcpy(p + 12, "IHDR", 4);
    put_be32(p + 16, uint32_t(lay.width));
    put_be32(p + 20, uint32_t(lay.height));
    p[24] = 8;  // bit depth
    p[25] = 2;  // colour type: RGB
    p[26] = p[27] = p[28] = 0;  // compression, filter method, no interlace
    put_be32(p + 29, mvlm_png_crc32(0, p + 12, 17));
    const size_t idat = 2 + payload_bytes + 4;
    put_be32(p + 33, uint32_t(idat));
    std::memcpy(p + 37, "IDAT", 4);
    p[41] = 0x78;
    p[42] = 0x01;
    uint8_t* q = file + HEAD_BYTES + payload_bytes;
    put_be32(q, adler);
    put_be32(q + 4, mvlm_png_crc32(0, p + 37, 4 + idat));
    put_be32(q + 8, 0);
    std::memcpy(q + 12, "IEND", 4);
    put_be32(q + 16, mvlm_png_crc32(0, q + 12, 4));
    *file_bytes = total;
    return 0;
}
