// raydrop_mlp.hip -- the tinycudann stand-in: frequency encoding and the bias-free fused MLP of the reference's ray-drop refinement
// network (scene/extre_train_raydrop.py), C ABI in include_tcnn/lidargs_tcnn.h.  The only source of liblidargs_tcnn.so: nothing here
// is linked into liblidargs_hip.so.  DESIGN.md section "tinycudann stand-in" has the layouts and the tile plan.
//
//   k_freq_fwd / k_freq_bwd   elementwise; t = scalbnf(x, f) is exact, sinpif / cospif of t never see a rounded product with pi.
//   k_mlp_fwd      one workgroup of 8 waves per 64 rows.  The row tile's activations live in one LDS image [64][132] between the
//                  layers; every layer is out[64,128] = act[64,K] W^T on v_mfma_f32_16x16x4_f32.  Wave w owns output columns
//                  16 w .. 16 w + 15 of all four 16-row tiles: a weight operand it fetches from L2 (one float4 per lane and 16 k) feeds
//                  four products.  The k index of a 16-k block is permuted (step s of lane group g is k = 16 kb + 4 g + s) so that both
//                  operands are 16-byte loads.
//   k_mlp_bwd      persistent workgroups (one per CU), grid-stride over 32-row tiles.  Nothing was saved: the tile's forward is
//                  recomputed into h + 1 LDS images (h_0 = x .. h_h), then the layers are walked backwards; delta_i overwrites h_i
//                  once h_i's values are dead.  The weight gradient of a tile, delta_i^T h_{i-1}, takes BOTH operands from LDS; each
//                  workgroup adds it into its own block of `partials` (plain stores on its first tile: the scratch needs no
//                  initialisation; the same lane owns the same element on every tile, so program order is all the ordering needed).
//   k_mlp_fold     dparams[p] = sum over the blocks in ascending order.  No atomics anywhere: results are bit-reproducible.
// Rows behind n are zero rows (x = 0 gives h = 0 without biases, dout = 0 gives delta = 0): masked in the loads and stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include_tcnn/lidargs_tcnn.h"
#include "lidargs_status.h"

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int WIDTH = LIDARGS_TCNN_WIDTH;
constexpr int LS = 132;                 // LDS row stride in floats: 16-byte rows, 4 r mod 64 banks apart
constexpr int DYS = 20;                 // row stride of the output layer's delta [rows][16]
constexpr int WAVES = 8;
constexpr int THREADS = 64 * WAVES;
constexpr int FWD_RT = 4;               // 16-row tiles per workgroup tile: forward 64 rows
constexpr int BWD_RT = 2;               //                                   backward 32 rows
constexpr int FREQ_THREADS = 256;
constexpr float PI_F = 3.14159265358979323846f;

__device__ __forceinline__ f4v mfma(float a, float b, f4v c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f4v zero4() { f4v c; c[0] = 0.f; c[1] = 0.f; c[2] = 0.f; c[3] = 0.f; return c; }

struct Mlp {
    int n, n_in, layers, n_out, out_act, aligned;
    const float* params;
    const float* x;
};

__device__ __forceinline__ size_t w_offset(const Mlp& m, int i) {          // W_i, i = 1 .. layers; layers + 1 is W_out
    return i == 1 ? 0 : (size_t)WIDTH * m.n_in + (size_t)(i - 2) * WIDTH * WIDTH;
}

// floats k .. k + 3 of row `row` of a row-major [nrows][K] matrix; zero outside (the K padding happens here, not in memory)
__device__ __forceinline__ float4 load_w4(const float* __restrict__ Wt, int row, int nrows, int K, int k, bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < nrows && k < K) {
        const float* p = Wt + (size_t)row * K + k;
        if (vec) v = *reinterpret_cast<const float4*>(p);                   // K % 4 == 0 and a 16-byte base: whole and aligned
        else {
            v.x = p[0];
            if (k + 1 < K) v.y = p[1];
            if (k + 2 < K) v.z = p[2];
            if (k + 3 < K) v.w = p[3];
        }
    }
    return v;
}

// rows row0 .. row0 + 16 RT - 1 of x into s[r][c], c < roundup16(n_in), zeros behind n and behind n_in
template <int RT>
__device__ __forceinline__ void stage_x(const Mlp& m, long long row0, float* s) {
    const int kp = (m.n_in + 15) & ~15;
    for (int i = threadIdx.x; i < 16 * RT * kp; i += THREADS) {
        const int r = i / kp, c = i - r * kp;
        const long long row = row0 + r;
        s[r * LS + c] = (row < m.n && c < m.n_in) ? m.x[(size_t)row * m.n_in + c] : 0.f;
    }
}

// The weight operands of dense_fwd for this wave's 16 output columns, all eight 16-k blocks in one round trip to L2.
__device__ __forceinline__ void load_fwd_w(const float* __restrict__ Wt, int K, bool vec, float4 (&b)[8]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int kb = 0; kb < 8; kb++) b[kb] = load_w4(Wt, 16 * wave + c, WIDTH, K, 16 * kb + 4 * g, vec);
}

// acc[rt] = act[16 rt .. +15][0 .. K) . Wt[16 wave .. +15][0 .. K)^T; Wt is [128][K] row-major (b: load_fwd_w), act's columns are zero up
// to roundup16(K)
template <int RT>
__device__ __forceinline__ void dense_fwd(const float* sIn, int K, const float4 (&b)[8], f4v (&acc)[RT]) {
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int rt = 0; rt < RT; rt++) acc[rt] = zero4();
#pragma unroll
    for (int kb = 0; kb < 8; kb++) {
        if (16 * kb < K) {                                                  // the same in every lane
            float4 a[RT];
#pragma unroll
            for (int rt = 0; rt < RT; rt++) a[rt] = *reinterpret_cast<const float4*>(sIn + (16 * rt + c) * LS + 16 * kb + 4 * g);
#pragma unroll
            for (int rt = 0; rt < RT; rt++) acc[rt] = mfma(a[rt].x, b[kb].x, acc[rt]);
#pragma unroll
            for (int rt = 0; rt < RT; rt++) acc[rt] = mfma(a[rt].y, b[kb].y, acc[rt]);
#pragma unroll
            for (int rt = 0; rt < RT; rt++) acc[rt] = mfma(a[rt].z, b[kb].z, acc[rt]);
#pragma unroll
            for (int rt = 0; rt < RT; rt++) acc[rt] = mfma(a[rt].w, b[kb].w, acc[rt]);
        }
    }
}

template <int RT>
__device__ __forceinline__ void store_relu(float* sOut, const f4v (&acc)[RT]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int e = 0; e < 4; e++) sOut[(16 * rt + 4 * g + e) * LS + 16 * wave + c] = fmaxf(acc[rt][e], 0.f);
}

// The output layer on the last hidden image: wave w < RT owns row tile w.  Forward: out = act(y) to global.  Backward (dout != NULL):
// delta_y = dout * act'(y) into sDY[r][o], zeros for o >= n_out and rows behind n.
template <int RT>
__device__ __forceinline__ void out_layer(const Mlp& m, const float* sIn, long long row0, float* __restrict__ out,
                                          const float* __restrict__ dout, float* sDY) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    if (wave >= RT) return;
    const float* Wt = m.params + w_offset(m, m.layers + 1);
    float4 b[8];
#pragma unroll
    for (int kb = 0; kb < 8; kb++) b[kb] = load_w4(Wt, c, m.n_out, WIDTH, 16 * kb + 4 * g, m.aligned != 0);
    f4v y[4] = {zero4(), zero4(), zero4(), zero4()};                        // four chains of 32 terms: the 16x16x4 form's dependent latency is
#pragma unroll                                                              // 40 cycles against 32 of issue, and shorter chains round less
    for (int kb = 0; kb < 8; kb++) {
        const float4 a = *reinterpret_cast<const float4*>(sIn + (16 * wave + c) * LS + 16 * kb + 4 * g);
        y[kb & 3] = mfma(a.x, b[kb].x, y[kb & 3]);
        y[kb & 3] = mfma(a.y, b[kb].y, y[kb & 3]);
        y[kb & 3] = mfma(a.z, b[kb].z, y[kb & 3]);
        y[kb & 3] = mfma(a.w, b[kb].w, y[kb & 3]);
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int r = 16 * wave + 4 * g + e;
        const long long row = row0 + r;
        const bool live = row < m.n && c < m.n_out;
        float v = (y[0][e] + y[1][e]) + (y[2][e] + y[3][e]);
        if (m.out_act == 1) v = 1.f / (1.f + expf(-v));
        if (dout == nullptr) {
            if (live) out[(size_t)row * m.n_out + c] = v;
        } else {
            float d = live ? dout[(size_t)row * m.n_out + c] : 0.f;
            if (m.out_act == 1) d *= v * (1.f - v);
            sDY[r * DYS + c] = d;
        }
    }
}

// The weight operands of dense_bwd_data for this wave's 16 output columns (Wt is [J][Kin] row-major), in one round trip to L2.
// Returns false for a wave whose columns lie behind Kin.
__device__ __forceinline__ bool load_bwd_w(const float* __restrict__ Wt, int J, int Kin, float (&b)[8][4]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int col = 16 * wave + c;
#pragma unroll
    for (int kb = 0; kb < 8; kb++)
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const int j = 16 * kb + 4 * g + s;
            b[kb][s] = (j < J && col < Kin) ? Wt[(size_t)j * Kin + col] : 0.f;
        }
    return 16 * wave < Kin;
}

// acc[rt] = sD[16 rt .. +15][0 .. J) . Wt[0 .. J)[16 wave .. +15] (b: load_bwd_w); sD's columns are zero up to roundup16(J).
template <int RT>
__device__ __forceinline__ void dense_bwd_data(const float* sD, int strideD, int J, const float (&b)[8][4], f4v (&acc)[RT]) {
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int rt = 0; rt < RT; rt++) acc[rt] = zero4();
#pragma unroll
    for (int kb = 0; kb < 8; kb++) {
        if (16 * kb < J) {
            float4 a[RT];
#pragma unroll
            for (int rt = 0; rt < RT; rt++) a[rt] = *reinterpret_cast<const float4*>(sD + (16 * rt + c) * strideD + 16 * kb + 4 * g);
#pragma unroll
            for (int rt = 0; rt < RT; rt++) acc[rt] = mfma(a[rt].x, b[kb][0], acc[rt]);
#pragma unroll
            for (int rt = 0; rt < RT; rt++) acc[rt] = mfma(a[rt].y, b[kb][1], acc[rt]);
#pragma unroll
            for (int rt = 0; rt < RT; rt++) acc[rt] = mfma(a[rt].z, b[kb][2], acc[rt]);
#pragma unroll
            for (int rt = 0; rt < RT; rt++) acc[rt] = mfma(a[rt].w, b[kb][3], acc[rt]);
        }
    }
}

// G[M][Nn] (+)= sA[rows][0 .. M)^T . sB[rows][0 .. Nn) over the tile's 16 RT rows: 16 x 16 tiles dealt to the waves round-robin, the
// reduction index of step (rt, s) is row 16 rt + 4 g + s.  sA's and sB's columns are readable (zero or dead) up to roundup16.
template <int RT>
__device__ __forceinline__ void weight_grad(const float* sA, int strideA, int M, const float* sB, int Nn, float* __restrict__ G, bool first) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int MT = (M + 15) >> 4, NT = (Nn + 15) >> 4;
    for (int p = wave; p < MT * NT; p += WAVES) {
        const int mt = p / NT, nt = p - mt * NT;
        float a[RT][4], b[RT][4];
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
#pragma unroll
            for (int s = 0; s < 4; s++) {
                a[rt][s] = sA[(16 * rt + 4 * g + s) * strideA + 16 * mt + c];
                b[rt][s] = sB[(16 * rt + 4 * g + s) * LS + 16 * nt + c];
            }
        f4v acc[2] = {zero4(), zero4()};
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
#pragma unroll
            for (int s = 0; s < 4; s++) acc[s & 1] = mfma(a[rt][s], b[rt][s], acc[s & 1]);
        const int nn = 16 * nt + c;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int mm = 16 * mt + 4 * g + e;
            if (mm < M && nn < Nn) {
                const size_t idx = (size_t)mm * Nn + nn;
                const float v = acc[0][e] + acc[1][e];
                G[idx] = first ? v : G[idx] + v;
            }
        }
    }
}

__global__ __launch_bounds__(THREADS) void k_mlp_fwd(const Mlp m, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_act[16 * FWD_RT * LS];
    const long long row0 = (long long)blockIdx.x * (16 * FWD_RT);
    stage_x<FWD_RT>(m, row0, s_act);
    __syncthreads();
    for (int i = 1; i <= m.layers; i++) {                                   // (three workgroups a CU hide the weights' round trip: no prefetch,
        float4 b[8];                                                        //  which would cost the third one its registers)
        load_fwd_w(m.params + w_offset(m, i), i == 1 ? m.n_in : WIDTH, i == 1 ? (m.aligned && !(m.n_in & 3)) : m.aligned != 0, b);
        f4v acc[FWD_RT];
        dense_fwd<FWD_RT>(s_act, i == 1 ? m.n_in : WIDTH, b, acc);
        __syncthreads();                                                    // every wave has read the whole image
        store_relu<FWD_RT>(s_act, acc);
        __syncthreads();
    }
    out_layer<FWD_RT>(m, s_act, row0, out, nullptr, nullptr);
}

__global__ __launch_bounds__(THREADS) void k_mlp_bwd(const Mlp m, const float* __restrict__ dout, float* __restrict__ dx,
                                                     float* __restrict__ partials, size_t n_params, int n_tiles) {
    extern __shared__ __attribute__((aligned(16))) float s_all[];
    constexpr int IMG = 16 * BWD_RT * LS;
    float* const sDY = s_all + (size_t)(m.layers + 1) * IMG;
    float* const G = partials + (size_t)blockIdx.x * n_params;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const bool vec1 = m.aligned && !(m.n_in & 3);
    bool first = true;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, first = false) {
        const long long row0 = (long long)tile * (16 * BWD_RT);
        {
            float4 b[8];
            load_fwd_w(m.params, m.n_in, vec1, b);
            stage_x<BWD_RT>(m, row0, s_all);
            __syncthreads();
            for (int i = 1; i <= m.layers; i++) {                           // the forward again: h_i into image i
                if (i > 1) load_fwd_w(m.params + w_offset(m, i), WIDTH, m.aligned != 0, b);
                f4v acc[BWD_RT];
                dense_fwd<BWD_RT>(s_all + (size_t)(i - 1) * IMG, i == 1 ? m.n_in : WIDTH, b, acc);
                store_relu<BWD_RT>(s_all + (size_t)i * IMG, acc);
                __syncthreads();
            }
        }
        float* sH = s_all + (size_t)m.layers * IMG;
        out_layer<BWD_RT>(m, sH, row0, nullptr, dout, sDY);
        __syncthreads();
        {                                                                   // the output layer: G_out = dY^T h_h, delta_h = (dY W_out) relu'(h_h)
            const size_t off = w_offset(m, m.layers + 1);
            weight_grad<BWD_RT>(sDY, DYS, m.n_out, sH, WIDTH, G + off, first);
            float b[8][4];
            load_bwd_w(m.params + off, m.n_out, WIDTH, b);
            f4v acc[BWD_RT];
            dense_bwd_data<BWD_RT>(sDY, DYS, m.n_out, b, acc);
            __syncthreads();                                                // h_h's values are dead
#pragma unroll
            for (int rt = 0; rt < BWD_RT; rt++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    float* q = sH + (16 * rt + 4 * g + e) * LS + 16 * wave + c;
                    *q = *q > 0.f ? acc[rt][e] : 0.f;
                }
            __syncthreads();
        }
        for (int i = m.layers; i >= 1; i--) {                               // image i holds delta_i, image i - 1 holds h_{i-1}
            const float* sD = s_all + (size_t)i * IMG;
            float* sP = s_all + (size_t)(i - 1) * IMG;
            const int Kin = i == 1 ? m.n_in : WIDTH;
            const size_t off = w_offset(m, i);
            weight_grad<BWD_RT>(sD, LS, WIDTH, sP, Kin, G + off, first);
            if (i == 1 && dx == nullptr) break;                             // (the next tile's staging is behind the barrier below)
            float b[8][4];
            const bool mine = load_bwd_w(m.params + off, WIDTH, Kin, b);
            f4v acc[BWD_RT];
            if (mine) dense_bwd_data<BWD_RT>(sD, LS, WIDTH, b, acc);
            if (i == 1) {
                if (mine) {
                    const int col = 16 * wave + c;
#pragma unroll
                    for (int rt = 0; rt < BWD_RT; rt++)
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const long long row = row0 + 16 * rt + 4 * g + e;
                            if (row < m.n && col < Kin) dx[(size_t)row * Kin + col] = acc[rt][e];
                        }
                }
                break;
            }
            __syncthreads();                                                // h_{i-1}'s values are dead
#pragma unroll
            for (int rt = 0; rt < BWD_RT; rt++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    float* q = sP + (16 * rt + 4 * g + e) * LS + 16 * wave + c;
                    *q = *q > 0.f ? acc[rt][e] : 0.f;
                }
            __syncthreads();
        }
        __syncthreads();                                                    // the images are free for the next tile
    }
}

__global__ __launch_bounds__(256) void k_mlp_fold(const float* __restrict__ partials, int blocks, size_t n_params, float* __restrict__ dparams) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_params) return;
    float s = 0.f;
    for (int b = 0; b < blocks; b++) s += partials[(size_t)b * n_params + p];
    dparams[p] = s;
}

__global__ __launch_bounds__(FREQ_THREADS) void k_freq_fwd(size_t total, int n_freq, const float* __restrict__ x, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * FREQ_THREADS + threadIdx.x;     // i = (row * dims + d) * F + f: the output pair's index
    if (i >= total) return;
    const size_t e = i / (size_t)n_freq;
    const int f = (int)(i - e * (size_t)n_freq);
    const float t = scalbnf(x[e], f);
    reinterpret_cast<float2*>(out)[i] = make_float2(sinpif(t), cospif(t));
}

__global__ __launch_bounds__(FREQ_THREADS) void k_freq_bwd(size_t elems, int n_freq, const float* __restrict__ x, const float* __restrict__ dout,
                                                           float* __restrict__ dx) {
    const size_t e = (size_t)blockIdx.x * FREQ_THREADS + threadIdx.x;     // e = row * dims + d
    if (e >= elems) return;
    const float xv = x[e];
    const float2* d = reinterpret_cast<const float2*>(dout) + e * (size_t)n_freq;
    float s = 0.f;
    for (int f = 0; f < n_freq; f++) {
        const float t = scalbnf(xv, f);
        const float2 dv = d[f];
        s += scalbnf(PI_F, f) * (cospif(t) * dv.x - sinpif(t) * dv.y);
    }
    dx[e] = s;
}

bool sizes_ok(int n_in, int layers, int n_out) {
    return n_in >= 1 && n_in <= WIDTH && layers >= 1 && layers <= LIDARGS_TCNN_MAX_HIDDEN_LAYERS && n_out >= 1 && n_out <= LIDARGS_TCNN_MAX_OUT;
}

size_t param_count(int n_in, int layers, int n_out) {
    return (size_t)WIDTH * n_in + (size_t)(layers - 1) * WIDTH * WIDTH + (size_t)n_out * WIDTH;
}

int compute_units() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
        (void)hipGetLastError();
        cus = 256;
    }
    return cus;
}

int bwd_tiles(int n) { return (int)(((long long)n + 16 * BWD_RT - 1) / (16 * BWD_RT)); }

int bwd_blocks(int n) {
    if (n <= 0) return 0;
    const int tiles = bwd_tiles(n), cus = compute_units();
    return tiles < cus ? tiles : cus;
}

}  // namespace

extern "C" {

int lidargs_tcnn_abi_version(void) { return LIDARGS_TCNN_ABI_VERSION; }
const char* lidargs_tcnn_last_error(void) { return g_err; }
int lidargs_tcnn_forward_row_tile(void) { return 16 * FWD_RT; }
int lidargs_tcnn_backward_row_tile(void) { return 16 * BWD_RT; }
int lidargs_tcnn_backward_blocks(int n) { return bwd_blocks(n); }

size_t lidargs_tcnn_param_count(int n_in, int n_hidden_layers, int n_out) {
    return sizes_ok(n_in, n_hidden_layers, n_out) ? param_count(n_in, n_hidden_layers, n_out) : 0;
}

size_t lidargs_tcnn_backward_partial_floats(int n, int n_in, int n_hidden_layers, int n_out) {
    return sizes_ok(n_in, n_hidden_layers, n_out) ? (size_t)bwd_blocks(n) * param_count(n_in, n_hidden_layers, n_out) : 0;
}

int lidargs_tcnn_frequency_forward(int n, int dims, int n_freq, const float* x, float* out, void* stream) {
    const char* what = "frequency_forward";
    if (n < 0 || dims < 1 || dims > WIDTH || n_freq < 1 || n_freq > LIDARGS_TCNN_MAX_FREQUENCIES) return fail(-1, what, "bad sizes");
    if (n == 0) return 0;
    if (!x || !out) return fail(-1, what, "NULL pointer with n > 0");
    if ((uintptr_t)out & 7) return fail(-1, what, "out must be 8-byte aligned");
    const size_t total = (size_t)n * dims * n_freq;
    const size_t blocks = (total + FREQ_THREADS - 1) / FREQ_THREADS;
    if (blocks > 0x7FFFFFFFull) return fail(-1, what, "too many elements for one call");
    hipLaunchKernelGGL(k_freq_fwd, dim3((unsigned)blocks), dim3(FREQ_THREADS), 0, (hipStream_t)stream, total, n_freq, x, out);
    return launched(-4, what);
}

int lidargs_tcnn_frequency_backward(int n, int dims, int n_freq, const float* x, const float* dout, float* dx, void* stream) {
    const char* what = "frequency_backward";
    if (n < 0 || dims < 1 || dims > WIDTH || n_freq < 1 || n_freq > LIDARGS_TCNN_MAX_FREQUENCIES) return fail(-1, what, "bad sizes");
    if (n == 0) return 0;
    if (!x || !dout || !dx) return fail(-1, what, "NULL pointer with n > 0");
    if ((uintptr_t)dout & 7) return fail(-1, what, "dout must be 8-byte aligned");
    const size_t elems = (size_t)n * dims;
    const size_t blocks = (elems + FREQ_THREADS - 1) / FREQ_THREADS;
    if (blocks > 0x7FFFFFFFull) return fail(-1, what, "too many elements for one call");
    hipLaunchKernelGGL(k_freq_bwd, dim3((unsigned)blocks), dim3(FREQ_THREADS), 0, (hipStream_t)stream, elems, n_freq, x, dout, dx);
    return launched(-4, what);
}

int lidargs_tcnn_mlp_forward(int n, int n_in, int n_hidden_layers, int n_out, int out_act, const float* params, const float* x,
                             float* out, void* stream) {
    const char* what = "mlp_forward";
    if (n < 0 || !sizes_ok(n_in, n_hidden_layers, n_out) || out_act < 0 || out_act > 1) return fail(-1, what, "bad sizes");
    if (n == 0) return 0;
    if (!params || !x || !out) return fail(-1, what, "NULL pointer with n > 0");
    const Mlp m = {n, n_in, n_hidden_layers, n_out, out_act, ((uintptr_t)params & 15) == 0, params, x};
    const unsigned blocks = (unsigned)(((long long)n + 16 * FWD_RT - 1) / (16 * FWD_RT));
    hipLaunchKernelGGL(k_mlp_fwd, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, m, out);
    return launched(-4, what);
}

int lidargs_tcnn_mlp_backward(int n, int n_in, int n_hidden_layers, int n_out, int out_act, const float* params, const float* x,
                              const float* dout, float* dparams, float* dx, float* partials, size_t partial_floats, void* stream) {
    const char* what = "mlp_backward";
    if (n < 0 || !sizes_ok(n_in, n_hidden_layers, n_out) || out_act < 0 || out_act > 1) return fail(-1, what, "bad sizes");
    if (!dparams) return fail(-1, what, "NULL dparams");
    if (n > 0 && (!params || !x || !dout)) return fail(-1, what, "NULL pointer with n > 0");
    const size_t n_params = param_count(n_in, n_hidden_layers, n_out);
    const int blocks = bwd_blocks(n);
    if (blocks > 0 && (!partials || partial_floats < (size_t)blocks * n_params)) return fail(-1, what, "partials too small");
    if (blocks > 0) {
        const Mlp m = {n, n_in, n_hidden_layers, n_out, out_act, ((uintptr_t)params & 15) == 0, params, x};
        const size_t lds = ((size_t)(n_hidden_layers + 1) * 16 * BWD_RT * LS + 16 * BWD_RT * DYS) * sizeof(float);
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_mlp_bwd), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return fail(-4, what, "LDS size: ", hipGetErrorString(e));
        hipLaunchKernelGGL(k_mlp_bwd, dim3((unsigned)blocks), dim3(THREADS), lds, (hipStream_t)stream, m, dout, dx, partials, n_params, bwd_tiles(n));
        if (const int rc = launched(-4, what)) return rc;
    }
    hipLaunchKernelGGL(k_mlp_fold, dim3((unsigned)((n_params + 255) / 256)), dim3(256), 0, (hipStream_t)stream, partials, blocks, n_params, dparams);
    return launched(-4, what, "fold launch: ");
}

}  // extern "C"
