// Stand-alone driver of mvlm_amd/csrc/png_pack.cpp for tests/test_png_pack_sanitized.py (built with -fsanitize=address,undefined).
//   harness IN OUT
// IN: cases, each u32 height, width, n_segments, then per segment u32 adler_a, adler_b, n_bytes and the bytes.  OUT: per case
// u32 file length and the file, assembled in a buffer of exactly the bound.  stdout: a line per case, then the bound
// function's answers at the corners and its refusals, and mvlm_png_finish's refusals.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../mvlm_amd/csrc/png_pack.h"

static bool read_u32(FILE* f, uint32_t* v) { return fread(v, 4, 1, f) == 1; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t h, w, nseg;
    int index = 0;
    while (read_u32(in, &h) && read_u32(in, &w) && read_u32(in, &nseg)) {
        mvlm_png::Layout lay;
        std::string why;
        if (mvlm_png_layout(int(h), int(w), lay, why)) {
            printf("case %d layout refused: %s\n", index, why.c_str());
            return 1;
        }
        if (uint32_t(lay.n_segments) != nseg) {
            printf("case %d INVARIANT segments %d != %u\n", index, lay.n_segments, nseg);
            return 1;
        }
        std::vector<uint8_t> file(lay.bound);
        std::vector<uint32_t> ab(2 * size_t(nseg));
        size_t payload = 0;
        for (uint32_t s = 0; s < nseg; ++s) {
            uint32_t n;
            if (!read_u32(in, &ab[2 * s]) || !read_u32(in, &ab[2 * s + 1]) || !read_u32(in, &n)) return 2;
            if (mvlm_png::HEAD_BYTES + payload + n > lay.bound - mvlm_png::TAIL_BYTES) {
                printf("case %d INVARIANT payload beyond the bound\n", index);
                return 1;
            }
            if (n && fread(file.data() + mvlm_png::HEAD_BYTES + payload, 1, n, in) != n) return 2;
            payload += n;
        }
        size_t bytes = 0;
        const uint32_t adler = mvlm_png_adler_combine(lay, ab.data());
        if (mvlm_png_finish(file.data(), file.size(), lay, payload, adler, &bytes, why)) {
            printf("case %d finish refused: %s\n", index, why.c_str());
            return 1;
        }
        const uint32_t len = uint32_t(bytes);
        fwrite(&len, 4, 1, out);
        fwrite(file.data(), 1, bytes, out);
        printf("case %d %ux%u segments %u payload %zu file %zu bound %zu adler %08x\n", index, h, w, nseg, payload, bytes, lay.bound, adler);
        // refusals of the assembly: a buffer one byte short, more payload than the layout allows, null pointers
        std::string r1, r2, r3;
        size_t dummy = 0;
        std::vector<uint8_t> tight(bytes - 1);
        std::memcpy(tight.data(), file.data(), bytes - 1);
        const int a = mvlm_png_finish(tight.data(), tight.size(), lay, payload, adler, &dummy, r1);
        const int b = mvlm_png_finish(file.data(), file.size(), lay, lay.payload_cap + 1, adler, &dummy, r2);
        const int c = mvlm_png_finish(nullptr, 0, lay, payload, adler, &dummy, r3);
        if (!a || !b || !c || r1.rfind("png:", 0) || r2.rfind("png:", 0) || r3.rfind("png:", 0)) {
            printf("case %d INVARIANT a refusal was taken\n", index);
            return 1;
        }
        ++index;
    }
    const int sizes[][2] = {{1, 1}, {4096, 4096}, {0, 1}, {1, 0}, {4097, 1}, {1, 4097}, {-1, -1}, {1 << 30, 1 << 30}};
    for (const auto& hw : sizes) {
        mvlm_png::Layout lay;
        std::string why;
        const int rc = mvlm_png_layout(hw[0], hw[1], lay, why);
        printf("bound %d %d rc=%d %zu %s\n", hw[0], hw[1], rc, rc ? size_t(0) : lay.bound, why.c_str());
    }
    const uint8_t check[9] = {'1', '2', '3', '4', '5', '6', '7', '8', '9'};
    printf("crc %08x\n", mvlm_png_crc32(0, check, 9));
    fclose(in);
    fclose(out);
    return 0;
}
