// thermal_agc.hip -- a thermal camera's automatic gain control: 16-bit counts -> 8-bit frames, on the device, integers only.
//
// A microbolometer delivers 14-16 bit counts of which a scene occupies a few hundred to a few thousand levels.
// ir2rgb_thermal_agc_u16 tone-maps N consecutive frames of one sequence, uint16 [N][H][W] -> uint8 [N][H][W][channels],
// with a histogram that is damped over time so that the gain does not flicker.  The definition is
// ir2rgb_amd.thermal.agc_reference (numpy, int64); the kernels equal it bit for bit, the state included.  Per frame,
// with P = H W, k = 65536 - a_q and >> an arithmetic shift (a floor):
//
//   h[v] = pixels equal to v                                            v = 0..65535
//   g[v] = min(h[v], plateau)  (plateau mode)    g[v] = h[v]  (linear mode)
//   S[v] = g[v] << 16                            on the first frame of a sequence,
//   S[v] = S[v] + ((((g[v] << 16) - S[v]) k) >> 16)                    afterwards          (Q16, int64)
//   C[v] = S[0] + ... + S[v],  T = C[65535]
//   plateau:  v0, v1 = smallest, largest v with S[v] > 0;  c0 = C[v0] (= S[v0]);  D = T - c0
//             lut[v] = (max(C[v] - c0, 0) 255 + D/2) / D,  all 0 when D == 0;  levels = (v0, v1)
//   linear:   lo = min{v : C[v] 10^6 > T tail_ppm},  hi = min{v : C[v] 10^6 >= T (10^6 - tail_ppm)},  Wd = hi - lo
//             lut[v] = clamp(((v - lo) 255 + Wd/2) / Wd, 0, 255),  all 0 when Wd == 0;  levels = (lo, hi)
//   out[p][c] = lut[x[p]]
//
// What the recurrence keeps (k in 1..65536): the step moves S toward g << 16 and never past it, so
// 0 <= S <= max(S_prev, g << 16) and sum S <= P 2^16; a level with pixels on it never reaches 0 (from S = 0 the step adds
// g k >= 1), so T > 0 always.  With P <= 2^26 (checked) every product stays below 2^62 -- (g << 16 - S) k < 2^42 2^16,
// C 10^6 < 2^42 2^20 -- and the plateau numerator below 2^50, which is why its division may go through fp64 (below).
//
// Three launches whatever the frames hold, no host synchronisation, no allocation:
//
//   agc_hist_kernel  grid (blocks, N), 1024 threads.  A thread reads 16 bytes = 8 pixels per trip (the frame's pixels before
//                    the first 16-byte boundary and behind the last whole vector are taken one by one by workgroup 0) and
//                    merges runs of equal neighbours.  Contention is the whole cost: a narrow scene puts 300 000 pixels on
//                    a thousand bins.  65536 dword bins are 256 KB, more than a workgroup's LDS, so no full private
//                    histogram exists; each workgroup keeps a WINDOW of 16384 bins (64 KB) in LDS, placed around the
//                    frame's first pixel, adds there with LDS atomics and flushes its non-zero bins with one global
//                    atomicAdd each at the end.  Levels outside the window go to the global bins at once, through
//                    wave_add: the lanes that hold the same level as the first such lane add up across the wave and make
//                    one atomicAdd.  Integer adds commute: the histogram is bit-reproducible.
//   agc_lut_kernel   ONE workgroup of 16 waves walks the frames in order (the recurrence is sequential).  A wave owns 4096
//                    consecutive levels and takes them in 16 trips of 256, four consecutive levels per lane, so every
//                    load and store is one contiguous kilobyte or more per wave.  Per frame: read the bins and ZERO THEM
//                    BEHIND ITSELF (the workspace is all zero on entry and on exit of every call: no memset launch), clip,
//                    update S in place, sum; the waves' sums go through LDS; v0/v1 by LDS min/max; then the running sum C
//                    by a wave scan per trip, lo/hi by LDS min, and the table.  A thread only ever reads the S it wrote
//                    itself.  The sequence-start flag is word 65536 of the state: tested, then set, here -- a captured
//                    graph replays correctly for the first and for every later frame, and reset() is a memset of that word.
//   agc_map_kernel   grid (blocks, N): gathers lut[n][x] (64 KB per frame; the occupied span stays in cache) and writes
//                    8 channels bytes per thread as 8-byte stores when the output is aligned where the input vectors start,
//                    else pixel by pixel.
#include "common.h"
#include "u8.h"         // or_byte

namespace {

constexpr int LEVELS = 65536;
constexpr int VEC = 8;                          // pixels of a 16-byte load
constexpr int HIST_BLOCK = 1024, HIST_TRIPS = 2, HIST_MAX_BLOCKS = 512;
constexpr int WINDOW = 16384;                   // bins a histogram workgroup keeps in LDS
constexpr int MAP_BLOCK = 256, MAP_MAX_BLOCKS = 1024;
constexpr int LUT_BLOCK = 1024;
constexpr int LUT_WAVES = LUT_BLOCK / IR2RGB_WAVE, WAVE_LEVELS = LEVELS / LUT_WAVES;      // 16 waves of 4096 levels
constexpr int LANE_LEVELS = 4, TRIP_LEVELS = IR2RGB_WAVE * LANE_LEVELS, LUT_TRIPS = WAVE_LEVELS / TRIP_LEVELS;
constexpr long MAX_PIXELS = 1L << 26;
enum { MODE_PLATEAU = 0, MODE_LINEAR = 1 };

typedef long long i64;
typedef __attribute__((ext_vector_type(2))) long long i64x2;

// pixels of the frame at f that lie before its first 16-byte boundary (f is 2-byte aligned), at most P
__device__ __forceinline__ int head_pixels(const void *f, int P) {
    const int h = (int)(((16u - (unsigned)((uintptr_t)f & 15u)) & 15u) >> 1);
    return h < P ? h : P;
}

__device__ __forceinline__ void unpack_u16(uint4 q, unsigned *v) {
    v[0] = q.x & 0xffffu, v[1] = q.x >> 16, v[2] = q.y & 0xffffu, v[3] = q.y >> 16;
    v[4] = q.z & 0xffffu, v[5] = q.z >> 16, v[6] = q.w & 0xffffu, v[7] = q.w >> 16;
}

// h[v] += c for every lane with flush; called by whole waves.  The lanes whose level equals the first flushing lane's are
// summed over the wave and added once.
__device__ __forceinline__ void wave_add(unsigned *h, unsigned v, unsigned c, bool flush) {
    const unsigned long long m = __ballot(flush);
    if (m == 0) return;                                         // (wave-uniform)
    const int lead = __ffsll(m) - 1;
    const unsigned first = __shfl(v, lead, IR2RGB_WAVE);
    const bool same = flush && v == first;
    unsigned tot = same ? c : 0u;
#pragma unroll
    for (int d = IR2RGB_WAVE / 2; d >= 1; d >>= 1) tot += __shfl_xor(tot, d, IR2RGB_WAVE);
    if ((int)(threadIdx.x & (IR2RGB_WAVE - 1)) == lead) atomicAdd(&h[first], tot);
    else if (flush && !same) atomicAdd(&h[v], c);
}

__global__ void __launch_bounds__(HIST_BLOCK)
agc_hist_kernel(const uint16_t *__restrict__ x, unsigned *__restrict__ hist, int P) {
    __shared__ unsigned win[WINDOW];
    const int n = blockIdx.y, tid = threadIdx.x;
    const uint16_t *f = x + (long)n * P;
    unsigned *h = hist + (long)n * LEVELS;
    int lo = (int)f[0] - WINDOW / 2;                            // the same window for all workgroups of the frame
    lo = lo < 0 ? 0 : (lo > LEVELS - WINDOW ? LEVELS - WINDOW : lo);
    for (int i = tid; i < WINDOW; i += HIST_BLOCK) win[i] = 0u;
    __syncthreads();
    const int head = head_pixels(f, P);
    const int nvec = (P - head) / VEC, tail = P - head - nvec * VEC;
    if (blockIdx.x == 0 && tid < head + tail) {                 // at most 7 + 7 pixels
        const int p = tid < head ? tid : nvec * VEC + tid;
        atomicAdd(&h[f[p]], 1u);
    }
    const uint4 *body = reinterpret_cast<const uint4 *>(f + head);
    for (int base = blockIdx.x * HIST_BLOCK; base < nvec; base += gridDim.x * HIST_BLOCK) {    // (base: wave-uniform)
        const int i = base + tid;
        const bool valid = i < nvec;
        unsigned v[VEC];
        unpack_u16(body[valid ? i : nvec - 1], v);
        unsigned cnt = 1;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const bool last = j == VEC - 1 || v[j] != v[j + 1 < VEC ? j + 1 : j];      // the run ends at j
            const unsigned w = v[j] - (unsigned)lo;
            const bool inside = w < (unsigned)WINDOW;
            if (valid && last && inside) atomicAdd(&win[w], cnt);
            wave_add(h, v[j], cnt, valid && last && !inside);
            cnt = last ? 1u : cnt + 1u;
        }
    }
    __syncthreads();
    for (int i = tid; i < WINDOW; i += HIST_BLOCK) {
        const unsigned c = win[i];
        if (c) atomicAdd(&h[lo + i], c);
    }
}

// floor(num / D) for 0 <= num < 2^53, 0 < D < 2^53 (both exact in fp64): the fp64 quotient is within one of it
__device__ __forceinline__ i64 floor_div53(i64 num, i64 D) {
    i64 q = (i64)((double)num / (double)D);
    if (q * D > num) --q;
    else if ((q + 1) * D <= num) ++q;
    return q;
}

// inclusive prefix sum over the lanes of a wave; whole waves only
__device__ __forceinline__ i64 wave_scan(i64 x, int lane) {
#pragma unroll
    for (int d = 1; d < IR2RGB_WAVE; d <<= 1) {
        const i64 t = __shfl_up(x, d, IR2RGB_WAVE);
        if (lane >= d) x += t;
    }
    return x;
}

__global__ void __launch_bounds__(LUT_BLOCK)
agc_lut_kernel(unsigned *__restrict__ hist, i64 *__restrict__ state, uint8_t *__restrict__ lut, int *__restrict__ levels,
               int N, int mode, unsigned plateau, int k, int tail_ppm) {
    __shared__ i64 s_wave[LUT_WAVES];                           // the waves' sums of S
    __shared__ i64 s_c0;
    __shared__ int s_a, s_b;                                    // v0, v1 or lo, hi
    const int tid = threadIdx.x, lane = tid & (IR2RGB_WAVE - 1), wave = tid / IR2RGB_WAVE;
    const int lb = wave * WAVE_LEVELS + lane * LANE_LEVELS;     // trip j: the four levels from lb + j TRIP_LEVELS
    i64 *S = state + lb;
    bool first = state[LEVELS] == 0;                            // the sequence starts with this call's frame 0
    __syncthreads();
    if (tid == 0) state[LEVELS] = 1;
    for (int n = 0; n < N; ++n, first = false) {
        unsigned *h = hist + (long)n * LEVELS + lb;
        if (tid == 0) s_a = LEVELS, s_b = mode == MODE_PLATEAU ? -1 : LEVELS;
        // ---- histogram -> S, the thread's sum, its first and last occupied level (its levels come in rising order)
        i64 sum = 0, c_first = 0;
        int v_first = LEVELS, v_last = -1;
#pragma unroll 4
        for (int j = 0; j < LUT_TRIPS; ++j) {
            const int o = j * TRIP_LEVELS;
            const uint4 q = *reinterpret_cast<const uint4 *>(h + o);
            *reinterpret_cast<uint4 *>(h + o) = make_uint4(0u, 0u, 0u, 0u);
            const unsigned hv[4] = {q.x, q.y, q.z, q.w};
            i64x2 s2[2] = {*reinterpret_cast<const i64x2 *>(S + o), *reinterpret_cast<const i64x2 *>(S + o + 2)};
#pragma unroll
            for (int u = 0; u < LANE_LEVELS; ++u) {
                const unsigned g = mode == MODE_PLATEAU ? min(hv[u], plateau) : hv[u];
                const i64 G = (i64)g << 16, old = s2[u >> 1][u & 1];
                const i64 s = first ? G : old + (((G - old) * k) >> 16);
                s2[u >> 1][u & 1] = s;
                sum += s;
                if (s > 0) {
                    if (v_first == LEVELS) v_first = lb + o + u, c_first = s;
                    v_last = lb + o + u;
                }
            }
            *reinterpret_cast<i64x2 *>(S + o) = s2[0];
            *reinterpret_cast<i64x2 *>(S + o + 2) = s2[1];
        }
        const i64 wave_sum = wave_scan(sum, lane);              // (lane 63 holds the wave's)
        if (lane == IR2RGB_WAVE - 1) s_wave[wave] = wave_sum;
        __syncthreads();                                        // s_a, s_b are set, s_wave is written
        i64 carry = 0, T = 0;                                   // C behind the levels before this wave's; the total
#pragma unroll
        for (int w = 0; w < LUT_WAVES; ++w) {
            const i64 t = s_wave[w];
            carry += w < wave ? t : 0;
            T += t;
        }
        uint8_t *row = lut + (long)n * LEVELS + lb;
        if (mode == MODE_PLATEAU) {
            if (v_last >= 0) atomicMin(&s_a, v_first), atomicMax(&s_b, v_last);
            __syncthreads();
            const int v0 = s_a, v1 = s_b;                       // T > 0: some level is occupied
            if (v_first == v0) s_c0 = c_first;                  // (one thread: the levels of two threads are disjoint)
            __syncthreads();
            const i64 c0 = s_c0, D = T - c0;
            for (int j = 0; j < LUT_TRIPS; ++j) {
                const int o = j * TRIP_LEVELS;
                const i64x2 a = *reinterpret_cast<const i64x2 *>(S + o), b = *reinterpret_cast<const i64x2 *>(S + o + 2);
                const i64 p[4] = {a[0], a[0] + a[1], a[0] + a[1] + b[0], a[0] + a[1] + b[0] + b[1]};
                const i64 incl = wave_scan(p[3], lane);
                const i64 before = carry + incl - p[3];
                carry += __shfl(incl, IR2RGB_WAVE - 1, IR2RGB_WAVE);
                unsigned w = 0u;
#pragma unroll
                for (int u = 0; u < LANE_LEVELS; ++u) {
                    const i64 up = before + p[u] - c0;
                    const unsigned y = D == 0 || up <= 0 ? 0u : (unsigned)floor_div53(up * 255 + D / 2, D);
                    w = or_byte(w, u, y);
                }
                *reinterpret_cast<unsigned *>(row + o) = w;
            }
            if (tid == 0) levels[2 * n] = v0, levels[2 * n + 1] = v1;
        } else {
            const i64 t_lo = T * tail_ppm, t_hi = T * (1000000 - tail_ppm);
            int lo = LEVELS, hi = LEVELS;
            for (int j = 0; j < LUT_TRIPS; ++j) {
                const int o = j * TRIP_LEVELS;
                const i64x2 a = *reinterpret_cast<const i64x2 *>(S + o), b = *reinterpret_cast<const i64x2 *>(S + o + 2);
                const i64 p[4] = {a[0], a[0] + a[1], a[0] + a[1] + b[0], a[0] + a[1] + b[0] + b[1]};
                const i64 incl = wave_scan(p[3], lane);
                const i64 before = carry + incl - p[3];
                carry += __shfl(incl, IR2RGB_WAVE - 1, IR2RGB_WAVE);
#pragma unroll
                for (int u = 0; u < LANE_LEVELS; ++u) {
                    const i64 c6 = (before + p[u]) * 1000000;
                    if (lo == LEVELS && c6 > t_lo) lo = lb + o + u;
                    if (hi == LEVELS && c6 >= t_hi) hi = lb + o + u;
                }
            }
            if (lo < LEVELS) atomicMin(&s_a, lo);
            if (hi < LEVELS) atomicMin(&s_b, hi);
            __syncthreads();
            lo = s_a, hi = s_b;                                 // both exist: C[65535] = T > 0
            const int Wd = hi - lo;
            for (int j = 0; j < LUT_TRIPS; ++j) {
                const int o = j * TRIP_LEVELS;
                unsigned w = 0u;
#pragma unroll
                for (int u = 0; u < LANE_LEVELS; ++u) {
                    const int v = lb + o + u;
                    unsigned y = 0u;
                    if (Wd > 0 && v > lo) y = v >= hi ? 255u : (unsigned)((v - lo) * 255 + Wd / 2) / (unsigned)Wd;
                    w = or_byte(w, u, y);
                }
                *reinterpret_cast<unsigned *>(row + o) = w;
            }
            if (tid == 0) levels[2 * n] = lo, levels[2 * n + 1] = hi;
        }
        __syncthreads();                                        // s_a, s_b, s_c0 and s_wave are free again
    }
}

template <int C>
__global__ void __launch_bounds__(MAP_BLOCK)
agc_map_kernel(const uint16_t *__restrict__ x, const uint8_t *__restrict__ lut, uint8_t *__restrict__ out, int P) {
    const int n = blockIdx.y, tid = threadIdx.x;
    const uint16_t *f = x + (long)n * P;
    const uint8_t *t = lut + (long)n * LEVELS;
    uint8_t *o = out + (long)n * P * C;
    int head = head_pixels(f, P);
    const bool wide = ((uintptr_t)(o + head * C) & 7u) == 0;   // 8 pixels are 8 C bytes: every vector's bytes are then aligned
    const int nvec = wide ? (P - head) / VEC : 0;
    if (!wide) head = 0;
    // pixels outside the vectors: [0, head) and [head + 8 nvec, P)
    for (int s = blockIdx.x * MAP_BLOCK + tid; s < P - nvec * VEC; s += gridDim.x * MAP_BLOCK) {
        const int p = s < head ? s : s + nvec * VEC;
        const uint8_t y = t[f[p]];
#pragma unroll
        for (int c = 0; c < C; ++c) o[p * C + c] = y;
    }
    const uint4 *body = reinterpret_cast<const uint4 *>(f + head);
    uint2 *dst = reinterpret_cast<uint2 *>(o + head * C);
    for (int i = blockIdx.x * MAP_BLOCK + tid; i < nvec; i += gridDim.x * MAP_BLOCK) {
        unsigned v[VEC], w[2 * C];
        unpack_u16(body[i], v);
#pragma unroll
        for (int j = 0; j < 2 * C; ++j) w[j] = 0u;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const unsigned y = t[v[j]];
#pragma unroll
            for (int c = 0; c < C; ++c) or_byte(w, j * C + c, y);
        }
#pragma unroll
        for (int j = 0; j < C; ++j) dst[i * C + j] = make_uint2(w[2 * j], w[2 * j + 1]);
    }
}

bool agc_sizes_ok(int N, int H, int W) {
    return N >= 1 && N <= 65535 && H >= 1 && W >= 1 && (long)H * W <= MAX_PIXELS;
}

int grid_blocks(int items, int per_block, int max_blocks) {
    const int b = cdiv(items, per_block);
    return b < 1 ? 1 : (b > max_blocks ? max_blocks : b);
}

}  // namespace

extern "C" long ir2rgb_thermal_agc_workspace_bytes(int N, int H, int W) {
    if (!agc_sizes_ok(N, H, W)) return IR2RGB_EINVAL;
    return (long)sizeof(unsigned) * LEVELS * N;
}

extern "C" int ir2rgb_thermal_agc_u16(const uint16_t *x, uint8_t *out, long long *state, uint8_t *lut, int *levels,
                                      void *workspace, long workspace_bytes, int N, int H, int W, int channels, int mode,
                                      int plateau, int a_q, int tail_ppm, void *stream) {
    if (!x || !out || !state || !lut || !levels || !workspace || !agc_sizes_ok(N, H, W)) return IR2RGB_EINVAL;
    if ((channels != 1 && channels != 3) || (mode != MODE_PLATEAU && mode != MODE_LINEAR) || plateau < 1) return IR2RGB_EINVAL;
    if (a_q < 0 || a_q > 65535 || tail_ppm < 0 || tail_ppm >= 500000) return IR2RGB_EINVAL;
    if (workspace_bytes < ir2rgb_thermal_agc_workspace_bytes(N, H, W)) return IR2RGB_EINVAL;
    if (misaligned(x, 2) || misaligned(state, 16) || misaligned(lut, 16) || misaligned(levels, 4) || misaligned(workspace, 16))
        return IR2RGB_EALIGN;
    const int P = H * W;
    hipStream_t s = as_stream(stream);
    unsigned *hist = static_cast<unsigned *>(workspace);
    agc_hist_kernel<<<dim3(grid_blocks(P / VEC, HIST_BLOCK * HIST_TRIPS, HIST_MAX_BLOCKS), N), HIST_BLOCK, 0, s>>>(x, hist, P);
    agc_lut_kernel<<<1, LUT_BLOCK, 0, s>>>(hist, state, lut, levels, N, mode, (unsigned)plateau, 65536 - a_q, tail_ppm);
    const int map_blocks = grid_blocks(P / VEC, MAP_BLOCK, MAP_MAX_BLOCKS);
    with_bool(channels == 3, [&](auto rgb) {
        agc_map_kernel<rgb.value ? 3 : 1><<<dim3(map_blocks, N), MAP_BLOCK, 0, s>>>(x, lut, out, P);
    });
    return ir2rgb_launch_status();
}
