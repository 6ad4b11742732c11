// PNG on the device (mvlm_png_encode): the pictures mvlm_render_landmark_view / mvlm_render_ray_view leave on the device, as
// complete 8-bit RGB PNG files in host memory, so that only compressed bytes cross to the host (DESIGN.md 4.5 holds the format
// contract; tests/png_model.py states it a second time and the GPU tests compare byte for byte).  Four kernels:
//   filter    one workgroup per row: the five filter types' costs (sum of b < 128 ? b : 256 - b) in one pass over the pixels,
//             the cheapest type (the lowest on a tie, or the forced one), the filtered row [type, 3 W bytes] in a second pass
//   deflate   one workgroup per 32 768-byte segment of an image's filtered stream, 128 bytes a thread: runs -> tokens (literals
//             and distance-1 matches), histograms in LDS, length-limited canonical Huffman lengths (the sort is a parallel
//             ranking, the tree and the header are thread 0's), the exact sizes of the stored, fixed and dynamic forms, the
//             smallest emitted by a prefix sum over the threads' bit counts; the Adler-32 partial sums of the segment
//   offsets   a thread per image: the running sum of its segments' sizes
//   gather    one workgroup per segment: its bytes to their place in the image's contiguous zlib payload
// The host side (layout, bound, Adler combination, chunks and CRC-32) is png_pack.cpp.  Every store is a plain C++ store or an
// atomicOr on a 32-bit word of a zeroed buffer.
#include "common.h"
#include "png_pack.h"

namespace {

using mvlm_png::SEGMENT;
constexpr int WG = 256;
constexpr int CHUNK = SEGMENT / WG;         // 128 bytes of the segment per thread
constexpr int PITCH_W = CHUNK / 4 + 1;      // LDS words per thread's chunk: 33, odd, so that the threads' byte reads spread over the banks
constexpr int SLOT = SEGMENT + 16;          // bytes of a segment's slot in scratch: its length + 10 at most, a multiple of 4
constexpr int NSYM = 286, NCL = 19, MAX_CL_ENTRIES = NSYM + 2;
constexpr int HDR_WORDS = 144;              // 17 + 19 * 3 + 288 * 14 bits at most
static_assert(SLOT % 4 == 0 && SLOT >= SEGMENT + int(mvlm_png::SEG_SLACK), "segment slot");

__constant__ const int CL_ORDER[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};  // RFC 1951 3.2.7

// ---- filter ---------------------------------------------------------------------------------------------------------------
__device__ inline int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ inline int predict(int type, int a, int b, int c) {
    return type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
}
__device__ inline int cost_of(int f) { return f < 128 ? f : 256 - f; }

__global__ __launch_bounds__(WG) void png_filter_kernel(const uchar4* __restrict__ rgba, int H, int W, int filter_mode,
                                                        uint8_t* __restrict__ stream) {
    __shared__ int s_cost[4][5];
    const int tid = threadIdx.x, r = blockIdx.x % H;
    const uchar4* const cur = rgba + size_t(blockIdx.x) * W;
    const uchar4* const up = cur - W;  // (read only when r > 0)
    const uchar4 zero = make_uchar4(0, 0, 0, 0);
    int type = filter_mode;
    if (filter_mode < 0) {
        int cost[5] = {0, 0, 0, 0, 0};
        for (int px = tid; px < W; px += WG) {
            const uchar4 x = cur[px], a = px > 0 ? cur[px - 1] : zero, b = r > 0 ? up[px] : zero, c = (r > 0 && px > 0) ? up[px - 1] : zero;
            const int xs[3] = {x.x, x.y, x.z}, as[3] = {a.x, a.y, a.z}, bs[3] = {b.x, b.y, b.z}, cs[3] = {c.x, c.y, c.z};
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int t = 0; t < 5; ++t) cost[t] += cost_of((xs[ch] - predict(t, as[ch], bs[ch], cs[ch])) & 255);
        }
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            int v = cost[t];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
            if ((tid & 63) == 0) s_cost[tid >> 6][t] = v;
        }
        __syncthreads();
        int best = 0x7FFFFFFF;
        type = 0;
        for (int t = 0; t < 5; ++t) {
            const int v = s_cost[0][t] + s_cost[1][t] + s_cost[2][t] + s_cost[3][t];
            if (v < best) {  // (strictly: the lowest type wins a tie)
                best = v;
                type = t;
            }
        }
    }
    uint8_t* const dst = stream + size_t(blockIdx.x) * (1 + 3 * size_t(W));
    if (tid == 0) dst[0] = uint8_t(type);
    for (int px = tid; px < W; px += WG) {
        const uchar4 x = cur[px], a = px > 0 ? cur[px - 1] : zero, b = r > 0 ? up[px] : zero, c = (r > 0 && px > 0) ? up[px - 1] : zero;
        dst[1 + 3 * px] = uint8_t(x.x - predict(type, a.x, b.x, c.x));
        dst[2 + 3 * px] = uint8_t(x.y - predict(type, a.y, b.y, c.y));
        dst[3 + 3 * px] = uint8_t(x.z - predict(type, a.z, b.z, c.z));
    }
}

// ---- deflate --------------------------------------------------------------------------------------------------------------
struct DeflateLds {
    uint32_t in[WG * PITCH_W];     // the segment, a thread's 128 bytes in 33 words
    int freq[NSYM + 2];            // literal/length histogram, then reused per alphabet
    int len[NSYM + 2];             // code lengths of the alphabet that is emitted
    uint32_t code[NSYM + 2];       // its codes, bit-reversed
    int sorted[NSYM + 2];          // symbols ascending by (count, symbol)
    int weight[2 * NSYM];          // leaves, then internal nodes in creation order
    int parent[2 * NSYM];          // parent links, then depths
    uint32_t cl[MAX_CL_ENTRIES];   // code-length symbols: symbol | extra value << 8
    int cl_freq[NCL], cl_len[NCL];
    uint32_t cl_code[NCL];
    uint32_t hdr[HDR_WORDS];       // the block header's bits
    int first[WG], last[WG];       // first / last run start in a thread's chunk; later the threads' bit counts
    int count[17], next[17];       // codes per length; the next code of a length
    int n_used, n_cl, kind, hdr_bits, dist_bits, size;
    uint32_t adler[2];
};

__device__ inline uint32_t in_byte(const DeflateLds& L, int p) {
    return (L.in[(p >> 7) * PITCH_W + ((p & 127) >> 2)] >> ((p & 3) * 8)) & 255u;
}

// length 3..258 -> symbol 257..285, its extra bits and their value (RFC 1951 3.2.5)
__device__ inline void length_symbol(int length, int* sym, int* ebits, int* eval) {
    const int l = length - 3;
    if (length == 258) {
        *sym = 285, *ebits = 0, *eval = 0;
    } else if (l < 8) {
        *sym = 257 + l, *ebits = 0, *eval = 0;
    } else {
        const int eb = 29 - __clz(l);  // floor(log2 l) - 2
        *sym = 261 + 4 * eb + ((l >> eb) & 3);
        *ebits = eb;
        *eval = l & ((1 << eb) - 1);
    }
}
__device__ inline int length_extra_bits(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }
__device__ inline int fixed_length(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }
__device__ inline uint32_t fixed_code(int sym) {
    return sym < 144 ? 0x30u + sym : sym < 256 ? 0x190u + (sym - 144) : sym < 280 ? uint32_t(sym - 256) : 0xC0u + (sym - 280);
}

// The tokens of the bytes [lo, hi) of the segment, in order: f(symbol, extra bits, extra value, is a match).  prev_start: the start of
// the run that holds byte lo - 1; next_start: the first run start at or behind hi (n when there is none).
template <class F>
__device__ inline void walk_tokens(const DeflateLds& L, int lo, int hi, int n, int prev_start, int next_start, F f) {
    int i = lo;
    int s = prev_start;
    while (i < hi) {
        const uint32_t v = in_byte(L, i);
        if (i == 0 || v != in_byte(L, i - 1)) s = i;
        int e = i + 1;
        while (e < hi && in_byte(L, e) == v) ++e;
        const int piece_end = e;                  // this thread's part of the run: [i, piece_end)
        if (e == hi) e = next_start;              // the run goes on (or ends) behind the chunk
        const int rest = e - s - 1;               // the run's bytes behind its first
        for (int p = i; p < piece_end; ++p) {
            const int k = p - s;
            if (k == 0) {
                f(int(v), 0, 0, false);
                continue;
            }
            const int j = k - 1, j0 = j / 258 * 258, piece = min(258, rest - j0);
            if (piece < 3) {
                f(int(v), 0, 0, false);
            } else if (j == j0) {
                int sym, eb, ev;
                length_symbol(piece, &sym, &eb, &ev);
                f(sym, eb, ev, true);
            }
        }
        i = piece_end;
    }
}

// Code lengths of at most `limit` bits for freq[0, nsym) into len[0, nsym): every thread calls it.  The symbols in use are ranked
// ascending by (count, symbol) in parallel; thread 0 builds the tree from two queues (leaves, internal nodes in creation order;
// the smaller head first, the leaf on a tie), counts the depths per length with the deeper ones at the limit, repairs the Kraft
// sum (one code leaves the limit, the deepest shorter code becomes two codes one bit longer) and deals the counts out over the
// ranking, the longest first; then the canonical codes, bit-reversed.
__device__ void build_code(DeflateLds& L, const int* freq, int nsym, int limit, int* len, uint32_t* code) {
    const int tid = threadIdx.x;
    if (tid == 0) L.n_used = 0;
    __syncthreads();
    for (int sym = tid; sym < nsym; sym += WG) {
        len[sym] = 0;
        code[sym] = 0;
        const int fq = freq[sym];
        if (fq > 0) {
            int rank = 0;
            for (int o = 0; o < nsym; ++o) {
                const int g = freq[o];
                rank += (g > 0 && (g < fq || (g == fq && o < sym))) ? 1 : 0;
            }
            L.sorted[rank] = sym;
            L.weight[rank] = fq;
            atomicAdd(&L.n_used, 1);
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int n = L.n_used;
        int* const count = L.count;
        int* const next = L.next;
        for (int l = 0; l < 17; ++l) count[l] = 0;
        if (n == 1) {
            count[1] = 1;
        } else if (n > 1) {
            int a = 0, b = n;
            for (int node = n; node < 2 * n - 1; ++node) {
                int w = 0;
                for (int k = 0; k < 2; ++k) {
                    int pick;
                    if (a < n && (b >= node || L.weight[a] <= L.weight[b])) pick = a++;
                    else pick = b++;
                    L.parent[pick] = node;
                    w += L.weight[pick];
                }
                L.weight[node] = w;
            }
            L.parent[2 * n - 2] = 0;  // the root's depth; every parent has a higher index than its children
            for (int node = 2 * n - 3; node >= 0; --node) {
                const int d = L.parent[L.parent[node]] + 1;
                L.parent[node] = d;
                if (node < n) count[min(d, limit)]++;
            }
            int total = 0;
            for (int l = 1; l <= limit; ++l) total += count[l] << (limit - l);
            while (total > (1 << limit)) {
                count[limit]--;
                for (int l = limit - 1; l > 0; --l)
                    if (count[l]) {
                        count[l]--;
                        count[l + 1] += 2;
                        break;
                    }
                --total;
            }
        }
        next[0] = next[1] = 0;
        {
            int c = 0;
            for (int l = 1; l <= limit; ++l) {
                c = (c + (l > 1 ? count[l - 1] : 0)) << 1;
                next[l] = c;
            }
        }
        int l = limit;
        for (int k = 0; k < n; ++k) {
            while (l > 1 && count[l] == 0) --l;
            len[L.sorted[k]] = l;
            count[l]--;
        }
        for (int sym = 0; sym < nsym; ++sym) {
            const int ln = len[sym];
            if (ln) code[sym] = __brev(uint32_t(next[ln]++)) >> (32 - ln);
        }
    }
    __syncthreads();
}

struct HeaderBits {
    uint32_t* words;
    int pos;
    __device__ void put(uint32_t v, int nb) {
        if (nb == 0) return;
        const int w = pos >> 5, o = pos & 31;
        words[w] |= v << o;
        if (o + nb > 32) words[w + 1] |= v >> (32 - o);
        pos += nb;
    }
};

__global__ __launch_bounds__(WG) void png_deflate_kernel(const uint8_t* __restrict__ stream, size_t stream_bytes, int n_seg,
                                                         int last_bytes, uint32_t* __restrict__ slots,
                                                         int32_t* __restrict__ seg_size, uint32_t* __restrict__ seg_adler) {
    __shared__ DeflateLds L;
    const int tid = threadIdx.x;
    const int img = blockIdx.x / n_seg, s = blockIdx.x % n_seg;
    const bool is_last = s + 1 == n_seg;
    const int n = is_last ? last_bytes : SEGMENT;
    const uint8_t* const src = stream + size_t(img) * stream_bytes + size_t(s) * SEGMENT;
    uint32_t* const dst = slots + size_t(blockIdx.x) * (SLOT / 4);
    uint8_t* const in8 = reinterpret_cast<uint8_t*>(L.in);

    for (int p = tid; p < n; p += WG) in8[(p >> 7) * (PITCH_W * 4) + (p & 127)] = src[p];
    for (int k = tid; k < NSYM + 2; k += WG) L.freq[k] = 0;
    for (int k = tid; k < HDR_WORDS; k += WG) L.hdr[k] = 0;
    if (tid < NCL) L.cl_freq[tid] = 0;
    if (tid < 2) L.adler[tid] = 0;
    __syncthreads();

    // ---- run starts per chunk, and the Adler-32 partial sums while the bytes pass ----
    const int lo = min(tid * CHUNK, n), hi = min(lo + CHUNK, n);
    {
        int first = 0x7FFFFFFF, last = -1;
        uint32_t a = 0, b = 0;
        uint32_t prev = lo > 0 ? in_byte(L, lo - 1) : 0;
        for (int i = lo; i < hi; ++i) {
            const uint32_t v = in_byte(L, i);
            if (i == 0 || v != prev) {
                if (last < 0) first = i;
                last = i;
            }
            prev = v;
            a += v;
            b += uint32_t(n - i) * v;  // (128 x 255 x 32768 at most: fits)
        }
        L.first[tid] = first;
        L.last[tid] = last;
        atomicAdd(&L.adler[0], a);  // (256 x 32 640 at most)
        atomicAdd(&L.adler[1], b % mvlm_png::ADLER_MOD);
    }
    __syncthreads();
    int prev_start = 0, next_start = n;
    for (int t = tid - 1; t >= 0; --t)
        if (L.last[t] >= 0) {
            prev_start = L.last[t];
            break;
        }
    for (int t = tid + 1; t < WG; ++t)
        if (L.first[t] != 0x7FFFFFFF) {
            next_start = L.first[t];
            break;
        }
    __syncthreads();  // (first / last are reused below)

    // ---- histogram ----
    walk_tokens(L, lo, hi, n, prev_start, next_start, [&](int sym, int, int, bool) { atomicAdd(&L.freq[sym], 1); });
    if (tid == 0) L.freq[256] = 1;
    __syncthreads();

    // ---- the dynamic form: lengths, header, sizes; the choice ----
    build_code(L, L.freq, NSYM, 15, L.len, L.code);
    if (tid == 0) {
        int n_match = 0;
        for (int k = 257; k < NSYM; ++k) n_match += L.freq[k];
        const int dist_len = n_match ? 1 : 0;
        int hlit = 257;
        for (int k = 257; k < NSYM; ++k)
            if (L.len[k]) hlit = k + 1;
        // the lengths (literal/length, then the one distance length) as code-length symbols
        int n_cl = 0;
        const int total = hlit + 1;
        int i = 0;
        while (i < total) {
            const int v = i < hlit ? L.len[i] : dist_len;
            int r = 1;
            while (i + r < total && (i + r < hlit ? L.len[i + r] : dist_len) == v) ++r;
            i += r;
            if (v == 0) {
                while (r >= 3) {
                    const int m = min(r, 138);
                    L.cl[n_cl++] = m >= 11 ? 18u | uint32_t(m - 11) << 8 : 17u | uint32_t(m - 3) << 8;
                    r -= m;
                }
            } else {
                L.cl[n_cl++] = uint32_t(v);
                --r;
                while (r >= 3) {
                    const int m = min(r, 6);
                    L.cl[n_cl++] = 16u | uint32_t(m - 3) << 8;
                    r -= m;
                }
            }
            for (; r > 0; --r) L.cl[n_cl++] = uint32_t(v);
        }
        for (int k = 0; k < n_cl; ++k) L.cl_freq[L.cl[k] & 255u]++;
        L.n_cl = n_cl;
        L.hdr_bits = hlit;  // (handed to the part below through LDS)
        L.dist_bits = dist_len;
    }
    __syncthreads();
    build_code(L, L.cl_freq, NCL, 7, L.cl_len, L.cl_code);
    if (tid == 0) {
        const int* const order = CL_ORDER;
        const int hlit = L.hdr_bits, n_cl = L.n_cl;
        int hclen = 4;
        for (int k = 4; k < NCL; ++k)
            if (L.cl_len[order[k]]) hclen = k + 1;
        HeaderBits h{L.hdr, 0};
        h.put(is_last ? 1u : 0u, 1);
        h.put(2u, 2);
        h.put(uint32_t(hlit - 257), 5);
        h.put(0u, 5);
        h.put(uint32_t(hclen - 4), 4);
        for (int k = 0; k < hclen; ++k) h.put(uint32_t(L.cl_len[order[k]]), 3);
        for (int k = 0; k < n_cl; ++k) {
            const int sym = int(L.cl[k] & 255u);
            const int eb = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
            h.put(L.cl_code[sym], L.cl_len[sym]);
            h.put(L.cl[k] >> 8, eb);
        }
        long long dyn = h.pos, fix = 3;
        int n_match = 0;
        for (int k = 0; k < NSYM; ++k) {
            const int fq = L.freq[k];
            if (!fq) continue;
            const int eb = k > 256 ? length_extra_bits(k) : 0;
            dyn += (long long)fq * (L.len[k] + eb);
            fix += (long long)fq * (fixed_length(k) + eb);
            if (k > 256) n_match += fq;
        }
        dyn += n_match;
        fix += 5LL * n_match;
        const long long stored_bytes = n + 5;
        const long long fix_bytes = is_last ? (fix + 7) / 8 : (fix + 3 + 7) / 8 + 4;
        const long long dyn_bytes = is_last ? (dyn + 7) / 8 : (dyn + 3 + 7) / 8 + 4;
        int kind = 0;
        long long best = stored_bytes;
        if (fix_bytes < best) kind = 1, best = fix_bytes;
        if (dyn_bytes < best) kind = 2, best = dyn_bytes;
        L.kind = kind;
        L.size = int(best);
        L.hdr_bits = kind == 2 ? h.pos : 3;
        L.dist_bits = kind == 2 ? 1 : 5;
        if (kind == 1) {
            for (int k = 0; k < HDR_WORDS; ++k) L.hdr[k] = 0;
            L.hdr[0] = (is_last ? 1u : 0u) | 1u << 1;
        }
        seg_size[blockIdx.x] = int(best);
        seg_adler[2 * blockIdx.x] = L.adler[0] % mvlm_png::ADLER_MOD;
        seg_adler[2 * blockIdx.x + 1] = L.adler[1] % mvlm_png::ADLER_MOD;
    }
    __syncthreads();
    const int kind = L.kind;

    // ---- stored: the header's five bytes, then the bytes ----
    if (kind == 0) {
        uint8_t* const d8 = reinterpret_cast<uint8_t*>(dst);
        if (tid == 0) {
            d8[0] = is_last ? 1 : 0;
            d8[1] = uint8_t(n & 255);
            d8[2] = uint8_t(n >> 8);
            d8[3] = uint8_t(~n & 255);
            d8[4] = uint8_t((~n >> 8) & 255);
        }
        for (int p = tid; p < n; p += WG) d8[5 + p] = uint8_t(in_byte(L, p));
        return;
    }
    if (kind == 1) {  // the fixed code in the tables' place
        for (int sym = tid; sym < NSYM; sym += WG) {
            const int ln = fixed_length(sym);
            L.len[sym] = ln;
            L.code[sym] = __brev(fixed_code(sym)) >> (32 - ln);
        }
        __syncthreads();
    }
    const int dist_bits = L.dist_bits, hdr_bits = L.hdr_bits;

    // ---- the threads' bit counts and their running sum ----
    {
        int bits = 0;
        walk_tokens(L, lo, hi, n, prev_start, next_start,
                    [&](int sym, int eb, int, bool match) { bits += L.len[sym] + eb + (match ? dist_bits : 0); });
        L.first[tid] = bits;
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < WG; ++t) {
            const int b = L.first[t];
            L.first[t] = run;
            run += b;
        }
    }
    __syncthreads();

    // ---- emit: the header's words, then every thread its tokens from its bit offset; the last thread ends the block ----
    for (int w = tid; w * 32 < hdr_bits; w += WG) atomicOr(&dst[w], L.hdr[w]);
    {
        int pos = hdr_bits + L.first[tid];
        int w = pos >> 5, fill = pos & 31;
        unsigned long long acc = 0;
        bool shared = true;  // the word under way may hold other threads' bits: the first one, and the last
        auto put = [&](uint32_t v, int nb) {
            acc |= (unsigned long long)v << fill;
            fill += nb;
            pos += nb;
            if (fill >= 32) {
                if (shared) atomicOr(&dst[w], uint32_t(acc));
                else dst[w] = uint32_t(acc);
                shared = false;
                acc >>= 32;
                fill -= 32;
                ++w;
            }
        };
        walk_tokens(L, lo, hi, n, prev_start, next_start, [&](int sym, int eb, int ev, bool match) {
            // code, extra bits, and for a match the distance code 0 (zeros): at most 15 + 5 + 5 bits
            put(L.code[sym] | uint32_t(ev) << L.len[sym], L.len[sym] + eb + (match ? dist_bits : 0));
        });
        if (tid == WG - 1) {
            put(L.code[256], L.len[256]);
            if (!is_last) {  // an empty stored block: 000, zeros to the byte boundary, 00 00 FF FF
                put(0u, 3);
                put(0u, (8 - (pos & 7)) & 7);
                put(0u, 16);
                put(0xFFFFu, 16);
            }
        }
        if (fill > 0) atomicOr(&dst[w], uint32_t(acc));
    }
}

// ---- gather ---------------------------------------------------------------------------------------------------------------
__global__ void png_offsets_kernel(const int32_t* __restrict__ seg_size, int n_images, int n_seg, uint32_t* __restrict__ seg_off,
                                   uint32_t* __restrict__ totals) {
    const int img = blockIdx.x * WG + threadIdx.x;
    if (img >= n_images) return;
    uint32_t run = 0;
    for (int s = 0; s < n_seg; ++s) {
        seg_off[size_t(img) * n_seg + s] = run;
        run += uint32_t(seg_size[size_t(img) * n_seg + s]);
    }
    totals[img] = run;
}

__global__ __launch_bounds__(WG) void png_gather_kernel(const uint32_t* __restrict__ slots, const int32_t* __restrict__ seg_size,
                                                        const uint32_t* __restrict__ seg_off, int n_seg, size_t payload_stride,
                                                        uint8_t* __restrict__ payload) {
    const int img = blockIdx.x / n_seg;
    const uint8_t* const src = reinterpret_cast<const uint8_t*>(slots + size_t(blockIdx.x) * (SLOT / 4));
    uint8_t* const dst = payload + size_t(img) * payload_stride + seg_off[blockIdx.x];
    const int n = seg_size[blockIdx.x];
    for (int p = threadIdx.x; p < n; p += WG) dst[p] = src[p];
}

}  // namespace

// ---- C ABI ----------------------------------------------------------------------------------------------------------------
extern "C" int mvlm_png_bound(int height, int width, size_t* bytes) {
    if (!bytes) return 2;
    mvlm_png::Layout lay;
    std::string why;
    if (mvlm_png_layout(height, width, lay, why)) return 1;
    *bytes = lay.bound;
    return 0;
}

extern "C" int mvlm_png_encode(mvlm_ctx* ctx, const uint8_t* rgba_dev, int n_images, int height, int width, int filter_mode,
                               uint8_t* png_host, size_t stride_bytes, size_t* png_bytes_out) {
    if (!ctx) return 1;
    MVLM_ENTER(ctx);
    ctx->png_clock.invalidate();
    MVLM_REQUIRE(ctx, rgba_dev && png_host && png_bytes_out, "png: null pointer");
    MVLM_REQUIRE(ctx, n_images >= 1 && n_images <= 128, "png: n_images must be 1..128 (" + std::to_string(n_images) + " given)");
    MVLM_REQUIRE(ctx, filter_mode >= -1 && filter_mode <= 4, "png: filter_mode must be -1..4 (" + std::to_string(filter_mode) + " given)");
    mvlm_png::Layout lay;
    std::string why;
    if (mvlm_png_layout(height, width, lay, why)) return ctx->fail(why);
    MVLM_REQUIRE(ctx, (long long)n_images * height * width <= 8LL * 2048 * 2048,
                 "png: n_images * height * width exceeds 8 * 2048 * 2048 pixels per call");
    MVLM_REQUIRE(ctx, stride_bytes >= lay.bound,
                 "png: stride_bytes " + std::to_string(stride_bytes) + " is below mvlm_png_bound's " + std::to_string(lay.bound));

    const size_t n_slots = size_t(n_images) * lay.n_segments;
    const size_t payload_stride = (lay.payload_cap + 15) / 16 * 16;
    auto* stream = static_cast<uint8_t*>(ctx->get_scratch("png.stream", size_t(n_images) * lay.stream_bytes));
    auto* slots = static_cast<uint32_t*>(ctx->get_scratch("png.slots", n_slots * SLOT));
    auto* payload = static_cast<uint8_t*>(ctx->get_scratch("png.payload", size_t(n_images) * payload_stride));
    // per segment: size, offset, the two Adler sums; per image: the total
    const size_t meta_words = 4 * n_slots + size_t(n_images);
    auto* meta = static_cast<uint32_t*>(ctx->get_scratch("png.meta", meta_words * 4));
    MVLM_REQUIRE(ctx, stream && slots && payload && meta, "png: scratch allocation failed");
    auto* seg_size = reinterpret_cast<int32_t*>(meta);
    uint32_t* const seg_off = meta + n_slots;
    uint32_t* const seg_adler = meta + 2 * n_slots;
    uint32_t* const totals = meta + 4 * n_slots;

    StageClock& clock = ctx->png_clock;
    if (clock.arm(ctx, 5)) return 1;
    hipStream_t st = ctx->stream;
    if (clock.record(ctx, 0, st)) return 1;
    hipLaunchKernelGGL(png_filter_kernel, dim3(unsigned(size_t(n_images) * height)), dim3(WG), 0, st,
                       reinterpret_cast<const uchar4*>(rgba_dev), height, width, filter_mode, stream);
    if (clock.record(ctx, 1, st)) return 1;
    MVLM_CHECK_HIP(ctx, hipMemsetAsync(slots, 0, n_slots * SLOT, st));  // (the deflate kernel ORs its bits in)
    hipLaunchKernelGGL(png_deflate_kernel, dim3(unsigned(n_slots)), dim3(WG), 0, st, stream, lay.stream_bytes, lay.n_segments,
                       int(lay.last_bytes), slots, seg_size, seg_adler);
    if (clock.record(ctx, 2, st)) return 1;
    hipLaunchKernelGGL(png_offsets_kernel, dim3(unsigned((n_images + WG - 1) / WG)), dim3(WG), 0, st, seg_size, n_images, lay.n_segments,
                       seg_off, totals);
    hipLaunchKernelGGL(png_gather_kernel, dim3(unsigned(n_slots)), dim3(WG), 0, st, slots, seg_size, seg_off, lay.n_segments,
                       payload_stride, payload);
    if (clock.record(ctx, 3, st)) return 1;
    MVLM_CHECK_HIP(ctx, hipGetLastError());

    std::vector<uint32_t> host_meta(meta_words);
    MVLM_CHECK_HIP(ctx, hipMemcpyAsync(host_meta.data(), meta, meta_words * 4, hipMemcpyDeviceToHost, st));
    MVLM_CHECK_HIP(ctx, hipStreamSynchronize(st));
    const uint32_t* const h_totals = host_meta.data() + 4 * n_slots;
    for (int i = 0; i < n_images; ++i) {
        MVLM_REQUIRE(ctx, h_totals[i] <= lay.payload_cap, "png: a payload exceeds its bound");
        MVLM_CHECK_HIP(ctx, hipMemcpyAsync(png_host + size_t(i) * stride_bytes + mvlm_png::HEAD_BYTES, payload + size_t(i) * payload_stride,
                                           h_totals[i], hipMemcpyDeviceToHost, st));
    }
    if (clock.record(ctx, 4, st)) return 1;
    MVLM_CHECK_HIP(ctx, hipStreamSynchronize(st));
    for (int i = 0; i < n_images; ++i) {
        const uint32_t adler = mvlm_png_adler_combine(lay, host_meta.data() + 2 * n_slots + 2 * size_t(i) * lay.n_segments);
        if (mvlm_png_finish(png_host + size_t(i) * stride_bytes, stride_bytes, lay, h_totals[i], adler, &png_bytes_out[i], why))
            return ctx->fail(why);
    }
    clock.mark(5);
    return 0;
}

extern "C" int mvlm_png_stage_ms(mvlm_ctx* ctx, float* ms4) {
    if (!ctx) return 1;
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, ms4, "png_stage_ms: null pointer");
    return ctx->png_clock.read(ctx, 4, ms4, "png_stage_ms: no picture was encoded with render profiling on");
}
