// Host side of the device PNG encoder (png_encode.hip): the segment layout of an image's filtered stream, the capacity bound,
// the Adler-32 of the stream from the segments' partial sums, and the file around the compressed bytes (signature, IHDR, one
// IDAT, IEND, a CRC-32 per chunk).  Plain C++ - no HIP - so that png_pack.cpp also builds with g++ -fsanitize=address,undefined
// for tests/test_png_pack_sanitized.py.  The format contract: DESIGN.md 4.5.
#ifndef MVLM_PNG_PACK_H
#define MVLM_PNG_PACK_H

#include <cstddef>
#include <cstdint>
#include <string>

namespace mvlm_png {

constexpr int SEGMENT = 32768;        // bytes of the filtered stream one workgroup compresses on its own
constexpr int MAX_DIM = 4096;         // height and width: 1..4096
constexpr size_t SEG_SLACK = 10;      // a segment's bytes beyond its length: 5 of a stored block's header, 5 of the flush
constexpr size_t HEAD_BYTES = 43;     // signature 8, IHDR 25, IDAT length and tag 8, zlib header 2: where the segments begin
constexpr size_t TAIL_BYTES = 20;     // Adler-32 4, IDAT's CRC 4, IEND 12
constexpr uint32_t ADLER_MOD = 65521;

struct Layout {
    int height = 0, width = 0;
    size_t row_bytes = 0;      // 1 + 3 * width: the filter type, then the filtered bytes
    size_t stream_bytes = 0;   // height * row_bytes
    int n_segments = 0;        // ceil(stream_bytes / SEGMENT); the last one holds last_bytes
    size_t last_bytes = 0;
    size_t payload_cap = 0;    // stream_bytes + n_segments * SEG_SLACK: what the segments' bytes can come to
    size_t bound = 0;          // HEAD_BYTES + payload_cap + TAIL_BYTES: what the file can come to
};

}  // namespace mvlm_png

// 0 and the layout, or 1 and why (every message starts with "png:"); never touches the GPU
int mvlm_png_layout(int height, int width, mvlm_png::Layout& out, std::string& why);
// Adler-32 of the whole stream from per-segment partials ab[2 s] = sum b mod 65521, ab[2 s + 1] = sum (n_s - i) b[i] mod 65521
// (the sums a segment has when it starts from A = 0, B = 0), in segment order
uint32_t mvlm_png_adler_combine(const mvlm_png::Layout& lay, const uint32_t* ab);
uint32_t mvlm_png_crc32(uint32_t crc, const uint8_t* data, size_t n);  // zlib's convention: start from 0
// The file around the segments' bytes, which lie at file + HEAD_BYTES already (payload_bytes of them): writes the head in
// front and Adler-32, the CRC and IEND behind.  1 and why when the capacity does not hold it or payload_bytes exceeds the layout's.
int mvlm_png_finish(uint8_t* file, size_t capacity, const mvlm_png::Layout& lay, size_t payload_bytes, uint32_t adler,
                    size_t* file_bytes, std::string& why);

#endif
