// azsp_hip.hip -- HIP / gfx950 backend of the engine: builds libazsp.so (the product).
// One workgroup = 256 threads = 4 wavefronts = 4 independent games (no inter-wave traffic, no
// __syncthreads); game g runs on block g/4, which the dispatcher places on XCD (g/4) % 8 in every
// launch, so a game's tree stays affine to one XCD's L2 across rounds.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <type_traits>

#include "azsp_impl.h"
#include "az_conv64.h"
#include "az_conv19.h"
#include "az_conv_sp.h"
#include "az_conv_sp17.h"
#include "az_resblock_sp17.h"
#include "az_conv_sp2p.h"
#include "az_conv_spg.h"

static hipError_t g_last = hipSuccess;
#define AZ_HIP(x) ((g_last = (x)) == hipSuccess ? 0 : -1)

template <int N, int GAME, class Op>
__global__ void __launch_bounds__(256) k_game(const AzCfg c, const AzMem m, const Op op, const int g0, const int g1) {
    __shared__ typename Engine<WaveDev, N, GAME>::SC sc[4];
    const int wave = (int)(threadIdx.x >> 6);
    const int g = g0 + (int)blockIdx.x * 4 + wave;  // games [g0, g1): a sub-range launch (g0 % 32 == 0) keeps every game on its XCD
    if (g >= g1) return;
    Engine<WaveDev, N, GAME> e(c, m, g, sc[wave]);
    op(e);
}

__global__ void __launch_bounds__(256) k_dihedral(const DihedralArgs a, long long total) {
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x)
        az_dihedral_elem(a, t);
}

__global__ void __launch_bounds__(256) k_replay_gather(const ReplayGatherArgs a, long long total) {
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x)
        az_replay_gather_elem(a, t);
}

__global__ void __launch_bounds__(256) k_replay_scatter(const ReplayAddArgs a, long long total) {
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x)
        az_replay_scatter_elem(a, t);
}

// One workgroup walks the rows in chunks of its size: thread t owns row base + t, the chunk's counts are scanned in LDS, the chunks' totals
// carried on (64-bit: ofs saturates, az_replay_ofs).
__global__ void __launch_bounds__(1024) k_replay_count(const float* __restrict__ weights, const double* __restrict__ unif, int* __restrict__ ofs, int n) {
    __shared__ long long sc[1024];
    const int t = (int)threadIdx.x;
    long long carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + t;
        const long long c = i < n ? az_replay_copies(weights[i], unif[i]) : 0;
        sc[t] = c;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {  // inclusive Hillis-Steele scan of the chunk's counts
            const long long a = t >= d ? sc[t - d] : 0;
            __syncthreads();
            sc[t] += a;
            __syncthreads();
        }
        if (i < n) ofs[i] = az_replay_ofs(carry + sc[t] - c);
        carry += sc[1023];
        __syncthreads();  // the next chunk overwrites sc
    }
    if (t == 0) ofs[n] = az_replay_ofs(carry);
}

__global__ void __launch_bounds__(256) k_bias_act(const BiasActArgs a) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.nvec; i += (long long)gridDim.x * blockDim.x)
        az_bias_act_vec(a, i);
}

// One workgroup: thread t owns a contiguous run of the rotated buffer order, the runs' totals are scanned in LDS.
__global__ void __launch_bounds__(1024) k_harvest_scan(const int* __restrict__ len, int* __restrict__ ofs, int* __restrict__ counts, int n2, int rot,
                                                        int cap, int max_games) {
    __shared__ int ss[1024], sg[1024], best[2];
    const int t = (int)threadIdx.x, per = (n2 + 1023) / 1024, lo = t * per < n2 ? t * per : n2, hi = lo + per < n2 ? lo + per : n2;
    int s = 0, g = 0;
    for (int i = lo; i < hi; ++i) {
        const int l = len[(i + rot) % n2];
        s += l;
        g += l > 0;
    }
    ss[t] = s;
    sg[t] = g;
    if (t < 2) best[t] = 0;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {  // inclusive Hillis-Steele scan of the run totals
        const int a = t >= d ? ss[t - d] : 0, b = t >= d ? sg[t - d] : 0;
        __syncthreads();
        ss[t] += a;
        sg[t] += b;
        __syncthreads();
    }
    int mine[2] = {0, 0};
    az_harvest_scan_range(len, ofs, n2, rot, cap, max_games, lo, hi, ss[t] - s, sg[t] - g, mine);
    if (mine[1] > 0) {  // the buffers that fit form a prefix of the order: the furthest fitting end is the harvest's total
        atomicMax(&best[0], mine[0]);
        atomicMax(&best[1], mine[1]);
    }
    __syncthreads();
    if (t < 2) counts[t] = best[t];
}

namespace azb {
void* alloc(size_t n) {
    void* p = nullptr;
    if (AZ_HIP(hipMalloc(&p, n))) return nullptr;
    if (AZ_HIP(hipMemset(p, 0, n))) {
        hipFree(p);
        return nullptr;
    }
    return p;
}
void release(void* p) { (void)hipFree(p); }
int h2d(void* d, const void* s, size_t n, void* st) {
    if (AZ_HIP(hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, (hipStream_t)st))) return -1;
    return AZ_HIP(hipStreamSynchronize((hipStream_t)st));  // the host buffer may be reused by the caller
}
int d2h(void* d, const void* s, size_t n, void* st) {
    if (AZ_HIP(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, (hipStream_t)st))) return -1;
    return AZ_HIP(hipStreamSynchronize((hipStream_t)st));
}
int zero(void* d, size_t n, void* st) { return AZ_HIP(hipMemsetAsync(d, 0, n, (hipStream_t)st)); }
int sync(void* st) { return AZ_HIP(hipStreamSynchronize((hipStream_t)st)); }
void* host_alloc(size_t n) {
    void* p = nullptr;
    return AZ_HIP(hipHostMalloc(&p, n, hipHostMallocDefault)) ? nullptr : p;
}
void host_release(void* p) { (void)hipHostFree(p); }
int set_device(int dev) {
    int n = 0;
    if (AZ_HIP(hipGetDeviceCount(&n)) || n < 1) return -1;
    return AZ_HIP(hipSetDevice(dev));
}
const char* backend_error() { return hipGetErrorString(g_last); }
// The three idioms of every launcher below.
// launch_k: enqueue on the caller's stream and report the launch error (0 / -1).
template <class K, class... A> static int launch_k(K* kernel, unsigned grid, unsigned block, size_t lds, void* st, const A&... args) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, (hipStream_t)st, args...);
    return AZ_HIP(hipGetLastError());
}
// with_flag: a run-time flag becomes a template parameter -- f(std::true_type) or f(std::false_type), a generic lambda whose parameter is
// usable as a template argument; the two-flag form nests it.
template <class F> static int with_flag(bool flag, F&& f) { return flag ? f(std::true_type{}) : f(std::false_type{}); }
template <class F> static int with_flag(bool f0, bool f1, F&& f) {
    return with_flag(f0, [&](auto F0) { return with_flag(f1, [&](auto F1) { return f(decltype(F0){}, F1); }); });
}
static int cu_count() {
    static int n_cu = 0;
    if (n_cu == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return -1;
        n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    return n_cu;
}
// persistent_grid: one persistent workgroup per CU, `k` CUs side by side on one unit of work (a tile, a board, a stripe of a board) and
// never more units in flight than there are; a device (partition) with < k CUs still gets one unit.  -1: the device cannot be queried.
static int persistent_grid(long long units, int k = 1) {
    const int n_cu = cu_count();
    if (n_cu < 0) return -1;
    const long long slots = n_cu / k > 0 ? n_cu / k : 1;
    return k * (int)(units < slots ? units : slots);
}
template <int N, int GAME, class Op> int launch(const AzCfg& c, const AzMem& m, const Op& op, void* st, int g0, int g1) {
    return launch_k(k_game<N, GAME, Op>, (unsigned)((g1 - g0 + 3) / 4), 256, 0, st, c, m, op, g0, g1);
}
int launch_dihedral(const DihedralArgs& a, long long total, void* st) {
    long long blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    return launch_k(k_dihedral, (unsigned)blocks, 256, 0, st, a, total);
}
int launch_replay_gather(const ReplayGatherArgs& a, long long total, void* st) {
    long long blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    return launch_k(k_replay_gather, (unsigned)blocks, 256, 0, st, a, total);
}
int launch_replay_count(const float* weights, const double* unif, int* ofs, int n, void* st) {
    return launch_k(k_replay_count, 1, 1024, 0, st, weights, unif, ofs, n);
}
int launch_replay_scatter(const ReplayAddArgs& a, long long total, void* st) {
    long long blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    return launch_k(k_replay_scatter, (unsigned)blocks, 256, 0, st, a, total);
}
int launch_harvest_scan(const int* len, int* ofs, int* counts, int n2, int rot, int cap, int max_games, void* st) {
    return launch_k(k_harvest_scan, 1, 1024, 0, st, len, ofs, counts, n2, rot, cap, max_games);
}
int launch_bias_act(const BiasActArgs& a, void* st) {
    long long blocks = (a.nvec + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;  // grid-stride beyond 32 blocks per CU
    return launch_k(k_bias_act, (unsigned)blocks, 256, 0, st, a);
}
int launch_conv3x3_tiled(const void* x, const void* w, const float* bias, const void* res, void* y, long long boards, int S, int C,
                         int relu, void* st, int f16) {
    if (f16 && (S != CV_S || C != CV_C)) return 1;  // f16 activations: the 9x9 x 128 kernels only
    const auto xb = (const unsigned char*)x, rb = (const unsigned char*)res;
    const auto wb = (const unsigned short*)w;
    const auto yb = (unsigned char*)y;
    if (C == C6_C && (S == 17 || S == 9)) {  // 64 filters: 17x17 planes (13x13 Gomoku network, one board per tile) or 9x9 Go (three boards per tile)
        const long long ntiles = S == 17 ? boards : (boards + 2) / 3;
        const int grid = persistent_grid(ntiles);
        if (grid < 0) return -1;
        return with_flag(S == 17, res != nullptr, [&](auto G17, auto RES) {
            return launch_k(k_conv3x3_t64<C6Geo<G17 ? 17 : 9>, RES, 8>, grid, CW_THREADS, 0, st, xb, wb, bias, rb, yb, (int)ntiles, relu);
        });
    }
    if (S == C9_S && C == 256) {  // 19x19 boards, 256 filters (jumbo Go network)
        // rounds 2-5's two-launch scheme, read once per process: the reference of the one-pass kernel's test, and its A/B partner
        static const bool two_launch = getenv("AZSP_CONV19_TWO_LAUNCH") != nullptr;
        const int grid = persistent_grid(boards, two_launch ? 4 : 8);
        if (grid < 0) return -1;
        if (x == y || res == y) return 1;  // other CUs read x's halo rows while y is written; the contract keeps the residual apart too
        if (!two_launch) {
            // ONE launch (round 6, k_conv3x3_op19q): a CU = 64 couts x all 256 cin of a half board, the four cin parts meet through LDS (half the
            // LDS fragment reads per flop of a two-way split), fp32 end to end; stripes of 8 workgroups (4 cout groups x 2 board halves) per tile stream
            return with_flag(res != nullptr, [&](auto RES) {
                return launch_k(k_conv3x3_op19q<RES>, grid, CW_THREADS, 0, st, xb, wb, bias, rb, yb, (int)boards, relu);
            });
        }
        // two launches, one per 128-channel half of the input; y holds the bf16 partial sum between them; stripes of 4 workgroups
        const int rc = with_flag(res != nullptr, [&](auto RES) {
            return launch_k(k_conv3x3_hb19<RES, 16>, grid, CW_THREADS, 0, st, xb, wb, bias, rb, yb, (int)boards, 0, 1, 256, 0, 32, 0);
        });
        if (rc) return rc;  // every launch is checked, not only the last one
        return launch_k(k_conv3x3_hb19<true, 16>, grid, CW_THREADS, 0, st, xb, wb, bias, (const unsigned char*)yb, yb, (int)boards, relu, 0, 256, 128, 32, 16);
    }
    if (S != CV_S || C != CV_C) return 1;
    const long long ntiles = (boards + CV_TB - 1) / CV_TB;
    const int grid = persistent_grid(ntiles);
    if (grid < 0) return -1;
    return with_flag(res != nullptr, f16 != 0, [&](auto RES, auto F16) {
        return launch_k(k_conv3x3_tiled<RES, 16, F16>, grid, CW_THREADS, 0, st, xb, wb, bias, rb, yb, (int)ntiles, relu);
    });
}
int launch_resblock_tiled(const void* x, const void* w1, const float* b1, const void* w2, const float* b2, void* y, long long boards, int S, int C,
                          void* st) {
    if (C != C6_C || (S != 17 && S != 9)) return 1;
    const long long ntiles = S == 17 ? boards : (boards + 2) / 3;
    const int grid = persistent_grid(ntiles);
    if (grid < 0) return -1;
    return with_flag(S == 17, [&](auto G17) {
        return launch_k(k_resblock64<C6Geo<G17 ? 17 : 9>>, grid, CW_THREADS, 0, st, (const unsigned char*)x, (const unsigned short*)w1, b1,
                        (const unsigned short*)w2, b2, (unsigned char*)y, (int)ntiles);
    });
}
int launch_stem_tiled(const void* x, const void* w, const float* bias, void* y, long long boards, int S, int C, int pad, int relu, void* st, int f16) {
    if (f16 && (S != CV_S || C != CV_C || pad != 1)) return 1;  // f16 activations: the 9x9 x 128 kernels only
    // Gomoku: 13x13 boards -> 17x17 planes; Go 9x9 x 64: three boards per tile; 19x19 Go: 17 planes (padded to 32) -> 256 filters, one launch
    const bool t64 = C == C6_C && ((S == 13 && pad == 3) || (S == 9 && pad == 1)), go19 = S == C9_S && C == 256 && pad == 1;
    if (!t64 && !go19 && (S != CV_S || C != CV_C || pad != 1)) return 1;
    const long long ntiles = t64 ? (S == 13 ? boards : (boards + 2) / 3) : go19 ? boards : (boards + CV_TB - 1) / CV_TB;
    const int grid = persistent_grid(ntiles, go19 ? 4 : 1);
    if (grid < 0) return -1;
    const auto xb = (const unsigned char*)x, nores = (const unsigned char*)nullptr;
    const auto wb = (const unsigned short*)w;
    const auto yb = (unsigned char*)y;
    if (t64)
        return with_flag(S == 13, [&](auto G17) {
            return launch_k(k_conv3x3_t64<C6Geo<G17 ? 17 : 9>, false, 4>, grid, CW_THREADS, 0, st, xb, wb, bias, nores, yb, (int)ntiles, relu);
        });
    if (go19) return launch_k(k_conv3x3_hb19<false, 4>, grid, CW_THREADS, 0, st, xb, wb, bias, nores, yb, (int)boards, relu, 1, 32, 0, 4, 0);
    return with_flag(f16 != 0, [&](auto F16) {
        return launch_k(k_conv3x3_tiled<false, 4, F16>, grid, CW_THREADS, 0, st, xb, wb, bias, nores, yb, (int)ntiles, relu);
    });
}
int launch_head_tiled(const void* x, const float* w, const float* bias, void* pol, void* val, long long boards, int S, int C, int npol, int nval,
                      int pol_stride, int val_stride, void* st, int f16) {
    if (C % 8 || C > 1024 || npol + nval != 3) return 1;
    const long long npos = boards * S * S;
    return with_flag(f16 != 0, [&](auto F16) {
        return launch_k(k_head_tiled<3, F16>, (unsigned)((npos + 255) / 256), 256, 0, st, (const unsigned char*)x, w, bias, (unsigned short*)pol,
                        (unsigned short*)val, npos, npol, C, S * S, cv_tile_boards(S) * S * S, pol_stride, val_stride);
    });
}
template <int T1, int T2, bool F16> static int launch_fc_heads_t(const FcHeadsArgs& a, void* st) {
    return launch_k(k_fc_heads<T1, T2, F16>, (unsigned)((a.boards + 127) / 128), 256, 0, st, (const unsigned short*)a.pol, (const unsigned short*)a.val,
                    (const unsigned short*)a.wp, a.bp, a.ks1, (const unsigned short*)a.w1, a.b1, a.ks2, a.w2, a.b2, a.priors, a.values, a.boards, a.A);
}
int launch_fc_heads(const FcHeadsArgs& a, void* st) {
    const int nt1 = (a.A + 31) / 32, nt2 = (a.F + 31) / 32;
    if (a.f16) return nt1 == 3 && nt2 == 4 ? launch_fc_heads_t<3, 4, true>(a, st) : 1;  // f16: the 9x9 x 128 evaluator (82 actions, 128 units)
    if (nt1 == 3 && nt2 == 2) return launch_fc_heads_t<3, 2, false>(a, st);
    if (nt1 == 3 && nt2 == 4) return launch_fc_heads_t<3, 4, false>(a, st);
    if (nt1 == 6 && nt2 == 2) return launch_fc_heads_t<6, 2, false>(a, st);
    if (nt1 == 6 && nt2 == 4) return launch_fc_heads_t<6, 4, false>(a, st);
    if (nt1 == 12 && nt2 == 8) return launch_fc_heads_t<12, 8, false>(a, st);
    return 1;
}
int launch_tile_layout(const void* src, void* dst, long long boards, int S, int C, int to_tiled, void* st) {
    if (C % 8 || S < 1) return 1;
    const int nch = C / 8, tile_rows = cv_tile_boards(S) * S * S;
    const long long nchunks = boards * S * S * nch;
    return launch_k(k_tile_layout, (unsigned)((nchunks + 255) / 256), 256, 0, st, (const unsigned char*)src, (unsigned char*)dst, nchunks, to_tiled, nch,
                    tile_rows);
}
int launch_split_layout(const void* src, void* dst, long long boards, int S, int C, int to_split, void* st, unsigned* range) {
    if (C % 8 || S < 1) return 1;
    const long long nchunks = boards * S * S * (C / 8);
    return launch_k(k_split_layout, (unsigned)((nchunks + 255) / 256), 256, 0, st, (const unsigned char*)src, (unsigned char*)dst, nchunks, to_split, C / 8,
                    S * S, range);
}
template <bool RES, int NCH, int NCG, bool XLO0 = false>
static int launch_sp(const void* x, const void* w, const float* bias, const void* res, void* y, long long boards, int relu, void* st, unsigned* range) {
    const int grid = persistent_grid(boards, NCG);  // the cout groups of a board run side by side
    if (grid < 0) return -1;
    return launch_k(k_conv3x3_sp<RES, NCH, NCG, XLO0>, grid, CW_THREADS, 0, st, (const unsigned char*)x, (const _Float16*)w, bias, (const unsigned char*)res,
                    (unsigned char*)y, (int)boards, relu, range);
}
template <bool RES, int NCH, bool XLO0 = false>
static int launch_sp17(const void* x, const void* w, const float* bias, const void* res, void* y, long long boards, int relu, void* st, unsigned* range) {
    const int grid = persistent_grid(boards);  // a board = two half-board tiles
    if (grid < 0) return -1;
    return launch_k(k_conv3x3_sp17<RES, NCH, XLO0>, grid, CW_THREADS, 0, st, (const unsigned char*)x, (const _Float16*)w, bias, (const unsigned char*)res,
                    (unsigned char*)y, (int)boards, relu, range);
}
// The wave-per-tile kernels of az_conv_spg.h: one WAVE per 16 NT couts x 16 NJ positions of an S x S plane, four waves per workgroup.
static long long spg_wave_items(long long boards, int S, int C, int NT, int NJ) {
    const long long nct = ((long long)S * S + 15) / 16;
    return boards * ((nct + NJ - 1) / NJ) * (C / (16 * NT));
}
// the grid of a launch of one wave per item; 0: too many for one launch
static unsigned spg_wave_grid(long long boards, int S, int C, int NT, int NJ) {
    const long long grid = (spg_wave_items(boards, S, C, NT, NJ) + 3) / 4;
    return grid > 0x7fffffffLL ? 0u : (unsigned)grid;
}
// k_conv3x3_spg: the fp32-class convolution with one WAVE per output tile -- any plane size, 64 / 128 / 256 filters.
// `latency`: small tiles (16 couts x 32 positions per wave) so that a handful of boards fill the chip; otherwise k_conv3x3_spgw:
// 16 NT couts x 48 positions per wave, the B fragments shared by the four waves of a workgroup through LDS.
// `halves` = 2 (latency only): k_conv3x3_sp2p's two accumulation chains (bit-identical to it at 9x9 x 128).
template <bool RES, int KSUB, int NT, int NJ, int HALVES>
static int launch_spg_t(const void* x, const void* w, const float* bias, const void* res, void* y, long long boards, int S, int C, int relu, void* st,
                        unsigned* range) {
    const unsigned grid = spg_wave_grid(boards, S, C, NT, NJ);
    if (!grid) return 1;
    return launch_k(k_conv3x3_spg<RES, KSUB, NT, NJ, HALVES>, grid, 256, 0, st, (const unsigned char*)x, (const _Float16*)w, bias,
                    (const unsigned char*)(RES ? res : nullptr), (unsigned char*)y, (int)boards, S, C, relu, range);
}
// large calls: the four waves of a workgroup share their B fragments through LDS (k_conv3x3_spgw; NT cout tiles per wave, C = 64 NT x groups)
template <bool RES, int KSUB, int NT>
static int launch_spgw_t(const void* x, const void* w, const float* bias, const void* res, void* y, long long boards, int S, int C, int relu, void* st,
                         unsigned* range) {
    const long long nct = ((long long)S * S + 15) / 16, grid = (boards * ((nct + 2) / 3) * (C / (64 * NT)) + 7) / 8 * 8;  // (a multiple of 8: XCD-aware order)
    if (grid > 0x7fffffffLL || C % (64 * NT)) return 1;
    return launch_k(k_conv3x3_spgw<RES, KSUB, NT>, (unsigned)grid, 256, 0, st, (const unsigned char*)x, (const _Float16*)w, bias,
                    (const unsigned char*)(RES ? res : nullptr), (unsigned char*)y, (int)boards, S, C, relu, range);
}
template <int KSUB, int HALVES>
static int launch_spg_k(const void* x, const void* w, const float* bias, const void* res, void* y, long long boards, int S, int C, int relu, void* st,
                        unsigned* range, bool latency) {
    constexpr int NT = KSUB == 2 ? 1 : 2;
    return with_flag(res != nullptr, [&](auto RES) {
        return latency || HALVES == 2 ? launch_spg_t<RES, KSUB, 1, 2, HALVES>(x, w, bias, res, y, boards, S, C, relu, st, range)
                                      : launch_spgw_t<RES, KSUB, NT>(x, w, bias, res, y, boards, S, C, relu, st, range);
    });
}
static int launch_spg(const void* x, const void* w, const float* bias, const void* res, void* y, long long boards, int S, int C, int relu, void* st,
                      unsigned* range, bool latency, int halves) {
    if (S < 3 || S > 64 || boards < 1 || boards > 0x7fffffffLL) return 1;
    if (C == 64) return launch_spg_k<2, 1>(x, w, bias, res, y, boards, S, C, relu, st, range, latency);
    if (C == 128)
        return halves == 2 ? launch_spg_k<4, 2>(x, w, bias, res, y, boards, S, C, relu, st, range, latency)
                           : launch_spg_k<4, 1>(x, w, bias, res, y, boards, S, C, relu, st, range, latency);
    if (C == 256) return launch_spg_k<8, 1>(x, w, bias, res, y, boards, S, C, relu, st, range, latency);
    return 1;
}
// Latency tiles (16 couts x 32 positions = one wave) per launch up to which the wave-per-tile kernel replaces a weight-stationary one of
// the same shape (bit-identical results; the weight-stationary kernels give a board to ONE workgroup: 10 - 33 us however few boards
// there are).  Default 1024 = one wave per SIMD of the chip: the measured crossover (tools/spg_ab.py, profiles/r06_spg_ab.txt: the kernel
// reads its fragments through L1, a second wave per SIMD doubles its time).  AZSP_SPG_MAX_WAVES sets the initial value (0 = never),
// azsp_small_batch_waves changes it at run time.
static constexpr long long SPG_DEFAULT_WAVES = 1024;
static long long& spg_max_waves() {
    static long long n = [] {
        const char* e = getenv("AZSP_SPG_MAX_WAVES");
        const long long v = e ? atoll(e) : SPG_DEFAULT_WAVES;
        return v < 0 ? 0LL : v;
    }();
    return n;
}
static bool small_batch(long long boards, int S, int C) { return spg_wave_items(boards, S, C, 1, 2) <= spg_max_waves(); }
long long small_batch_waves(long long n) {
    const long long old = spg_max_waves();
    if (n >= 0) spg_max_waves() = n;
    return old;
}
int launch_conv3x3_split(const void* x, const void* w, const float* bias, const void* res, void* y, long long boards, int S, int C, int relu,
                         void* st, unsigned* range) {
    const bool sp17 = S == Sp17Geo::S && C == 64, sp9 = S == SpGeo9::S && (C == 128 || C == 64), small = small_batch(boards, S, C);
    // no tailored (weight-stationary) kernel for the shape, or a handful of boards: one wave per tile; at 9x9 x 128 in k_conv3x3_sp2p's summation order
    if (!(sp17 || sp9) || small) return launch_spg(x, w, bias, res, y, boards, S, C, relu, st, range, small, sp9 && C == 128 ? 2 : 1);
    if (sp17)  // 17x17 planes x 64 filters: the 13x13 Gomoku tower (half-board tiles)
        return with_flag(res != nullptr, [&](auto RES) { return launch_sp17<RES, 8>(x, w, bias, res, y, boards, relu, st, range); });
    if (C == 64) return with_flag(res != nullptr, [&](auto RES) { return launch_sp<RES, 8, 1>(x, w, bias, res, y, boards, relu, st, range); });
    // 9x9 x 128: k_conv3x3_sp2p (az_conv_sp2p.h): the 2 x 2 split of a CU's work between its waves (half the LDS fragment reads per MFMA), one
    // workgroup iteration per PAIR of adjacent boards, without the MFMAs that only multiply the zero padding.  It runs the first boards / 2
    // pairs; an odd last board runs the wave-per-tile kernel on offset pointers (bit-identical; whatever the small-batch limit is, also 0).
    const long long pairs = boards / 2;
    const int pgrid = persistent_grid(pairs, 2);
    if (pgrid < 0) return -1;
    const size_t off = (size_t)(2 * pairs) * 2 * 128 * SpGeo9::P2 * 2;  // bytes of 2 * pairs boards in the split layout
    const auto xb = (const unsigned char*)x, rb = (const unsigned char*)res;
    const auto yb = (unsigned char*)y;
    const int rc = with_flag(res != nullptr, [&](auto RES) {
        return pairs > 0 ? launch_k(k_conv3x3_sp2p<RES>, pgrid, CW_THREADS, 0, st, xb, (const _Float16*)w, bias, rb, yb, (int)pairs, relu, range) : 0;
    });
    if (rc || !(boards & 1)) return rc;
    return launch_spg(xb + off, w, bias, res ? rb + off : nullptr, yb + off, 1, S, C, relu, st, range, true, 2);
}
// Lazily allocated scratch, one buffer per purpose and device, never freed.  Calls on different streams of one device that need the same
// buffer would share it -- the evaluator runs one stream per network.
enum Scratch {
    SCRATCH_SPG_BLOCK,  // the intermediate activations of azsp_resblock_split on a handful of boards: SPG_SCRATCH_BOARDS boards of 17x17 x 64
    SCRATCH_COUNT
};
static constexpr long long SPG_SCRATCH_BOARDS = 256;
static void* device_scratch(Scratch which, size_t bytes) {
    static void* buf[SCRATCH_COUNT][16] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
    if (!buf[which][dev] && AZ_HIP(hipMalloc(&buf[which][dev], bytes))) return nullptr;
    return buf[which][dev];
}
// A ResNetBlock of up to SPG_SCRATCH_BOARDS boards x 64 filters as two wave-per-tile convolutions (az_conv_spg.h) through the block scratch:
// conv1 with ReLU into the scratch, conv2 with the residual x into y -- bit-identical to the fused block.  The scratch is sized once for
// SPG_SCRATCH_BOARDS boards of 17x17 (19 MB), whoever asks first: a process that only ever meets the odd last 9x9 board allocates it too
// (that tail had a 20 KB buffer of its own).
static int launch_resblock_spg(const unsigned char* x, const void* w1, const float* b1, const void* w2, const float* b2, unsigned char* y, long long boards,
                               int S, int C, void* st, unsigned* range) {
    void* mid = device_scratch(SCRATCH_SPG_BLOCK, (size_t)SPG_SCRATCH_BOARDS * 2 * 8 * Sb17::S * Sb17::S * 16);
    if (!mid) return -1;
    const int rc = launch_spg(x, w1, b1, nullptr, mid, boards, S, C, 1, st, range, true, 1);
    if (rc) return rc;
    return launch_spg(mid, w2, b2, x, y, boards, S, C, 1, st, range, true, 1);
}
int launch_resblock_split(const void* x, const void* w1, const float* b1, const void* w2, const float* b2, void* y, long long boards, int S, int C,
                          void* st, unsigned* range) {
    if (C != 64 || (S != Sb17::S && S != Sb9::S)) return 1;  // 17x17 planes (the 13x13 Gomoku tower) or 9x9 planes (9x9 Go, logs/go/9x9_12b64) x 64 filters
    const long long pairs = boards / 2;  // 9x9: the fused kernel takes blocks of TWO boards
    const int grid = persistent_grid(S == Sb9::S ? pairs : boards);  // 17x17: a board = two half-board tiles x two phases
    if (grid < 0) return -1;
    const auto xb = (const unsigned char*)x;
    const auto yb = (unsigned char*)y;
    // a handful of boards: the wave-per-tile convolutions instead of one workgroup per board
    if (small_batch(boards, S, C) && boards <= SPG_SCRATCH_BOARDS) return launch_resblock_spg(xb, w1, b1, w2, b2, yb, boards, S, C, st, range);
    // the fused block: one launch per ResNetBlock; at 9x9 on the first boards / 2 pairs, and an odd last board runs as the handful above
    if (S == Sb17::S) return launch_k(k_resblock_sp<Sb17, 6>, grid, CW_THREADS, 0, st, xb, (const _Float16*)w1, b1, (const _Float16*)w2, b2, yb, (int)boards, range);
    if (pairs > 0 && launch_k(k_resblock_sp<Sb9, 6>, grid, CW_THREADS, 0, st, xb, (const _Float16*)w1, b1, (const _Float16*)w2, b2, yb, (int)pairs, range)) return -1;
    if (!(boards & 1)) return 0;
    const size_t off = (size_t)(boards - 1) * Sb9::GTILEB;
    return launch_resblock_spg(xb + off, w1, b1, w2, b2, yb + off, 1, S, C, st, range);
}
int launch_split_features(const float* src, void* dst, long long boards, int S, int cin, void* st, unsigned* range) {
    if (cin < 1 || cin > 32 || S < 1) return 1;
    const long long nitems = boards * 4 * S * S;
    return launch_k(k_split_features, (unsigned)((nitems + 255) / 256), 256, 0, st, src, (unsigned char*)dst, nitems, cin, S * S, range);
}
// k_stem_spg (az_conv_spg.h): the stem with one WAVE per output tile (16 couts x 32 positions) -- any board, pad 1 or 3, 64 / 128 / 256 filters
template <bool XLO0>
static int launch_stem_spg(const void* x, const void* w, const float* bias, void* y, long long boards, int n, int C, int pad, int relu, void* st,
                           unsigned* range) {
    constexpr int NT = 1, NJ = 2;
    const int off = pad - 1, S = n + 2 * off;
    if ((pad != 1 && pad != 3) || n < 1 || S < 3 || S > 64 || (C != 64 && C != 128 && C != 256) || boards < 1 || boards > 0x7fffffffLL) return 1;
    const unsigned grid = spg_wave_grid(boards, S, C, NT, NJ);
    if (!grid) return 1;
    return launch_k(k_stem_spg<XLO0, NT, NJ>, grid, 256, 0, st, (const unsigned char*)x, (const _Float16*)w, bias, (unsigned char*)y, (int)boards, n, off,
                    C, relu, range);
}
// S: the BOARD (the output planes are S + 2 (pad - 1) wide).  The three tailored shapes run their weight-stationary stems unless the call
// is small (small_batch on the output plane, as the tower: bit-identical results); every other shape runs the wave-per-tile stem.
// The DEFAULT threshold does not move the tailored shapes (STEM_SPG_DEFAULT_SMALL): they switch only when the caller has raised it.
static constexpr bool STEM_SPG_DEFAULT_SMALL = false;
int launch_stem_split(const void* x, const void* w, const float* bias, void* y, long long boards, int S, int C, int pad, int relu, void* st,
                      int x_lo_zero, unsigned* range) {
    const bool sp17 = S == 13 && C == 64 && pad == 3;  // 13x13 boards -> 17x17 planes
    const bool sp9 = S == SpGeo9::S && (C == 128 || C == 64) && pad == 1;
    const bool small = (pad == 1 || pad == 3) && small_batch(boards, S + 2 * (pad - 1), C) && (STEM_SPG_DEFAULT_SMALL || spg_max_waves() > SPG_DEFAULT_WAVES);
    return with_flag(x_lo_zero != 0, [&](auto XLO0) {
        if (!(sp17 || sp9) || small) return launch_stem_spg<XLO0>(x, w, bias, y, boards, S, C, pad, relu, st, range);
        if (sp17) return launch_sp17<false, 4, XLO0>(x, w, bias, nullptr, y, boards, relu, st, range);
        return C == 128 ? launch_sp<false, 4, 2, XLO0>(x, w, bias, nullptr, y, boards, relu, st, range)
                        : launch_sp<false, 4, 1, XLO0>(x, w, bias, nullptr, y, boards, relu, st, range);
    });
}
int split_range_read(const unsigned* rec, unsigned out[2], int reset, void* st) {
    void* p = (void*)rec;  // null: the per-device default record
    if (!p && AZ_HIP(hipGetSymbolAddress(&p, HIP_SYMBOL(g_sp_range)))) return -1;
    if (AZ_HIP(hipMemcpyAsync(out, p, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, (hipStream_t)st))) return -1;
    if (reset && AZ_HIP(hipMemsetAsync(p, 0, 2 * sizeof(unsigned), (hipStream_t)st))) return -1;
    return AZ_HIP(hipStreamSynchronize((hipStream_t)st));
}
template <int BPB> static int launch_head_split_bpb(const HeadSplitArgs& a, void* st) {
    const int P2 = a.S * a.S;
    const size_t lds = (size_t)(BPB * (3 * ((P2 + 3) & ~3) + a.A + a.F)) * sizeof(float);
    if (lds > 64 * 1024) return 1;
    return launch_k(k_head_split<BPB>, (unsigned)((a.boards + BPB - 1) / BPB), 256, lds, st, (const unsigned char*)a.x, a.hw, a.hb, a.wp_t, a.bp, a.w1_t, a.b1, a.w2,
                    a.b2, a.priors, a.values, a.boards, a.C, P2, a.A, a.F, a.npol);
}
int launch_head_split(const HeadSplitArgs& a, void* st) {
    if (a.C % 8 || a.npol < 1 || a.npol > 2) return 1;
    return launch_head_split_bpb<4>(a, st);  // (8 boards per workgroup: measured slower, see k_head_split)
}
}  // namespace azb
