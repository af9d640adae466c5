// decode_options.hip -- the feature bank and the per-camera appearance embedding in front of the fused anchor decode
// (C ABI in include_decode/lidargs_decode_options.h).  The only source of liblidargs_decode_options.so: nothing here is linked into
// liblidargs_hip.so, and no kernel of neural_gaussians.hip is touched -- the decode reads feat' where it read the anchor feature,
// and a packed W1 with a folded bias where it read the colour and ray-drop heads' first layer.
//
//   k_bank_forward    (:37-47)  EIGHT LANES own one anchor: lane l of the group holds feat[4l .. 4l+3] as one float4 (a wave moves
//                     eight whole 128-byte rows per load), computes hidden units 4l .. 4l+3 of the bank MLP from the group's
//                     (view, dist) and its share of the three logits; the group's sums are two DPP quad permutes and a half-row
//                     mirror (no LDS crossbar).  The strided sources feat[4 (j mod 8)] and feat[2 (j mod 16)] of the lane's four
//                     outputs are the .x / .z components of other lanes of the group: eight shuffles, no second read.  140 B read +
//                     128 B written per visible anchor.  Measured at 2.4 TB/s of those bytes: a round is flag -> rows -> a chain of
//                     cross-lane sums, so the kernel is latency- rather than bandwidth-limited.
//   k_bank_backward   the same layout; recomputes w, takes dw = sum_j g[j] source[j] with the forward's shuffles, back-propagates
//                     the softmax and the MLP inside the group, and gathers dL_dfeat from the group's row of g staged in LDS
//                     (feat[m] feeds outputs m, {m/4 + 8r} and {m/2 + 16s}).  Each lane keeps its 35 parameter sums (its four hidden
//                     units' rows of dW1, db1, columns of dW2; db2) in registers over the workgroup's anchors; at the end they are added
//                     across the groups of a wave (shuffles), across the four waves (LDS, in wave order) and written as ONE row of
//                     `partials` per workgroup.  268 B read + 140 B written per visible anchor.
//   k_bank_fold       dL_dparams = the sum of the rows, in a fixed order (a wave per parameter).  No float atomics, no waiting on another workgroup.
//   k_appearance_fold / k_appearance_backward   one small launch each: a thread per element.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include_decode/lidargs_decode_options.h"
#include "lidargs_status.h"

namespace {

constexpr int BK_THREADS = 256;
constexpr int BK_GROUP = 8;                            // lanes per anchor
constexpr int BK_ANCHORS = BK_THREADS / BK_GROUP;      // anchors per workgroup and round
constexpr int BK_FEAT = 32;
constexpr int BK_ROW = BK_FEAT + 4;                    // LDS row of g: padded by one float4
constexpr int BK_ACC = 35;                             // a lane's parameter sums: dW1 4x4 | db1 4 | dW2 3x4 | db2 3
constexpr int BK_PARAMS = LIDARGS_NG_BANK_PARAMS;
constexpr int BK_FWD_MAX_BLOCKS = 2048;
constexpr int BK_BWD_MAX_BLOCKS = 1024;                // = the most rows of `partials`
static_assert(BK_PARAMS == 128 + 32 + 96 + 3, "W1 | b1 | W2 | b2");

// A lane's share of the bank MLP: hidden units 4l .. 4l+3.
struct BankLane { float w1[4][4]; float b1[4]; float w2[3][4]; float b2[3]; };

__device__ __forceinline__ BankLane bank_lane(const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2,
                                              const float* __restrict__ b2, int l) {
    BankLane m;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const float4 r = *reinterpret_cast<const float4*>(W1 + 4 * (4 * l + u));
        m.w1[u][0] = r.x; m.w1[u][1] = r.y; m.w1[u][2] = r.z; m.w1[u][3] = r.w;
        m.b1[u] = b1[4 * l + u];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float4 r = *reinterpret_cast<const float4*>(W2 + 32 * c + 4 * l);
        m.w2[c][0] = r.x; m.w2[c][1] = r.y; m.w2[c][2] = r.z; m.w2[c][3] = r.w;
        m.b2[c] = b2[c];
    }
    return m;
}

// The sum over the 8 lanes of a group, the same bits in every lane, without a trip through the LDS crossbar: lane ^ 1 and lane ^ 2 by
// quad permutes, then the other quad of the group by mirroring the row's halves (lane l <-> 7 - l).
template <int CTRL> __device__ __forceinline__ float bk_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float group_sum(float v) {
    v += bk_dpp<0xB1>(v);                                              // quad_perm [1,0,3,2]
    v += bk_dpp<0x4E>(v);                                              // quad_perm [2,3,0,1]
    v += bk_dpp<0x141>(v);                                             // row_half_mirror
    return v;
}

// (view, dist) of an anchor (:28-34) and the bank weights w (:40); h = the lane's four ReLU outputs.
__device__ __forceinline__ void bank_weights(const BankLane& m, const float (&x)[4], float (&h)[4], float (&w)[3]) {
    float part[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 4; u++) {
        float acc = m.b1[u];
#pragma unroll
        for (int q = 0; q < 4; q++) acc += m.w1[u][q] * x[q];
        h[u] = fmaxf(acc, 0.f);
#pragma unroll
        for (int c = 0; c < 3; c++) part[c] += m.w2[c][u] * h[u];
    }
    float z[3];
#pragma unroll
    for (int c = 0; c < 3; c++) z[c] = group_sum(part[c]) + m.b2[c];
    const float top = fmaxf(z[0], fmaxf(z[1], z[2]));                  // nn.Softmax(dim=1): exp(z - max) / sum
    const float e0 = expf(z[0] - top), e1 = expf(z[1] - top), e2 = expf(z[2] - top);
    const float s = e0 + e1 + e2;
    w[0] = e0 / s; w[1] = e1 / s; w[2] = e2 / s;
}

// The strided sources of the lane's outputs j = 4l + c:  a[c] = feat[4 (j mod 8)] = .x of lane 4 (l & 1) + c of the group,
// b[c] = feat[2 (j mod 16)] = .x (c even) or .z (c odd) of lane 2 (l & 3) + c / 2.
__device__ __forceinline__ void bank_sources(const float4& f, int l, float (&a)[4], float (&b)[4]) {
    const int a0 = 4 * (l & 1), b0 = 2 * (l & 3);
#pragma unroll
    for (int c = 0; c < 4; c++) a[c] = __shfl(f.x, a0 + c, BK_GROUP);
    b[0] = __shfl(f.x, b0, BK_GROUP); b[1] = __shfl(f.z, b0, BK_GROUP);
    b[2] = __shfl(f.x, b0 + 1, BK_GROUP); b[3] = __shfl(f.z, b0 + 1, BK_GROUP);
}

__device__ __forceinline__ void bank_view(const float* __restrict__ anchor, size_t i, float3 cam, bool vis, float (&x)[4]) {
    float ox = 1.f, oy = 0.f, oz = 0.f;                                // (an invisible anchor's lanes take part in the shuffles with finite values)
    if (vis) { ox = anchor[3 * i] - cam.x; oy = anchor[3 * i + 1] - cam.y; oz = anchor[3 * i + 2] - cam.z; }
    const float dist = sqrtf(ox * ox + oy * oy + oz * oz);
    x[0] = ox / dist; x[1] = oy / dist; x[2] = oz / dist; x[3] = dist;
}

__global__ void __launch_bounds__(BK_THREADS) k_bank_forward(int N, const uint8_t* __restrict__ mask, const float* __restrict__ feat,
                                                             const float* __restrict__ anchor, float3 cam, const float* __restrict__ W1,
                                                             const float* __restrict__ b1, const float* __restrict__ W2,
                                                             const float* __restrict__ b2, float* __restrict__ out) {
    const int l = threadIdx.x & (BK_GROUP - 1), grp = threadIdx.x / BK_GROUP;
    const BankLane m = bank_lane(W1, b1, W2, b2, l);
    const int rounds = (N + BK_ANCHORS - 1) / BK_ANCHORS;
    for (int r = blockIdx.x; r < rounds; r += gridDim.x) {
        const size_t i = (size_t)r * BK_ANCHORS + grp;
        const bool in = i < (size_t)N;
        const bool vis = in && (!mask || mask[i]);
        float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
        if (vis) f = *reinterpret_cast<const float4*>(feat + i * BK_FEAT + 4 * l);
        float x[4], h[4], w[3], a[4], b[4];
        bank_view(anchor, i, cam, vis, x);
        bank_weights(m, x, h, w);
        bank_sources(f, l, a, b);
        float4 o;
        o.x = a[0] * w[0] + b[0] * w[1] + f.x * w[2];                  // (:44-46, in the reference's order)
        o.y = a[1] * w[0] + b[1] * w[1] + f.y * w[2];
        o.z = a[2] * w[0] + b[2] * w[1] + f.z * w[2];
        o.w = a[3] * w[0] + b[3] * w[1] + f.w * w[2];
        if (!vis) o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (in) *reinterpret_cast<float4*>(out + i * BK_FEAT + 4 * l) = o;
    }
}

__global__ void __launch_bounds__(BK_THREADS, 4) k_bank_backward(int N, const uint8_t* __restrict__ mask, const float* __restrict__ feat,
                                                              const float* __restrict__ anchor, float3 cam, const float* __restrict__ W1,
                                                              const float* __restrict__ b1, const float* __restrict__ W2,
                                                              const float* __restrict__ b2, const float* __restrict__ g_out,
                                                              float* __restrict__ d_feat, float* __restrict__ d_anchor,
                                                              float* __restrict__ partials) {
    __shared__ __attribute__((aligned(16))) float s_g[BK_ANCHORS * BK_ROW];
    __shared__ float s_red[(BK_THREADS / 64) * BK_GROUP * BK_ACC];
    const int l = threadIdx.x & (BK_GROUP - 1), grp = threadIdx.x / BK_GROUP;
    const BankLane m = bank_lane(W1, b1, W2, b2, l);
    float acc[BK_ACC];
#pragma unroll
    for (int q = 0; q < BK_ACC; q++) acc[q] = 0.f;
    const int rounds = (N + BK_ANCHORS - 1) / BK_ANCHORS;              // (the trip count is the workgroup's: the barriers below are reached by all)
    // A round's loads are requested one round ahead: the visible flag, then the two rows behind it, are two dependent round trips that
    // would otherwise stand in front of every round's arithmetic.
    bool nvis = false;
    float4 nf = make_float4(0.f, 0.f, 0.f, 0.f), ng = nf;
    auto request = [&](int r) {
        const size_t i = (size_t)r * BK_ANCHORS + grp;
        nvis = r < rounds && i < (size_t)N && (!mask || mask[i]);
        nf = make_float4(0.f, 0.f, 0.f, 0.f); ng = nf;
        if (nvis) {
            nf = *reinterpret_cast<const float4*>(feat + i * BK_FEAT + 4 * l);
            ng = *reinterpret_cast<const float4*>(g_out + i * BK_FEAT + 4 * l);
        }
    };
    request(blockIdx.x);
    for (int r = blockIdx.x; r < rounds; r += gridDim.x) {
        const size_t i = (size_t)r * BK_ANCHORS + grp;
        const bool in = i < (size_t)N;
        const bool vis = nvis;
        const float4 f = nf, g = ng;
        request(r + gridDim.x);
        float* row = s_g + grp * BK_ROW;
        *reinterpret_cast<float4*>(row + 4 * l) = g;
        float x[4], h[4], w[3], a[4], b[4];
        bank_view(anchor, i, cam, vis, x);
        bank_weights(m, x, h, w);
        bank_sources(f, l, a, b);
        // dL/dw, then through the softmax: dz_c = w_c (dw_c - sum_c' w_c' dw_c')
        float dw[3];
        dw[0] = group_sum(g.x * a[0] + g.y * a[1] + g.z * a[2] + g.w * a[3]);
        dw[1] = group_sum(g.x * b[0] + g.y * b[1] + g.z * b[2] + g.w * b[3]);
        dw[2] = group_sum(g.x * f.x + g.y * f.y + g.z * f.z + g.w * f.w);
        const float mean = w[0] * dw[0] + w[1] * dw[1] + w[2] * dw[2];
        float dz[3], dx[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; c++) { dz[c] = w[c] * (dw[c] - mean); acc[32 + c] += dz[c]; }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            float dh = 0.f;
#pragma unroll
            for (int c = 0; c < 3; c++) { dh += m.w2[c][u] * dz[c]; acc[20 + 4 * c + u] += dz[c] * h[u]; }
            const float d1 = h[u] > 0.f ? dh : 0.f;                    // ReLU
            acc[16 + u] += d1;
#pragma unroll
            for (int q = 0; q < 4; q++) { acc[4 * u + q] += d1 * x[q]; dx[q] += m.w1[u][q] * d1; }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) dx[q] = group_sum(dx[q]);
        __syncthreads();                                               // the group's row of g is in s_g
        // feat[m] feeds output m (weight w2); m = 4l also outputs l, l+8, l+16, l+24 (w0); m = 4l and 4l+2 also outputs m/2, m/2+16 (w1)
        const float s0 = row[l] + row[l + 8] + row[l + 16] + row[l + 24];
        const float2 p0 = *reinterpret_cast<const float2*>(row + 2 * l), p1 = *reinterpret_cast<const float2*>(row + 2 * l + 16);
        float4 df;
        df.x = g.x * w[2] + s0 * w[0] + (p0.x + p1.x) * w[1];
        df.y = g.y * w[2];
        df.z = g.z * w[2] + (p0.y + p1.y) * w[1];
        df.w = g.w * w[2];
        if (!vis) df = make_float4(0.f, 0.f, 0.f, 0.f);
        if (in) {
            *reinterpret_cast<float4*>(d_feat + i * BK_FEAT + 4 * l) = df;
            if (l == 0) {
                // view = o / dist, dist = |o|:  dL/do = (dview - view (view . dview)) / dist + ddist view
                const float vd = x[0] * dx[0] + x[1] * dx[1] + x[2] * dx[2];
                float ax = (dx[0] - x[0] * vd) / x[3] + dx[3] * x[0];
                float ay = (dx[1] - x[1] * vd) / x[3] + dx[3] * x[1];
                float az = (dx[2] - x[2] * vd) / x[3] + dx[3] * x[2];
                if (!vis) { ax = 0.f; ay = 0.f; az = 0.f; }
                d_anchor[3 * i] = ax; d_anchor[3 * i + 1] = ay; d_anchor[3 * i + 2] = az;
            }
        }
        __syncthreads();                                               // s_g is free for the next round
    }
    // the workgroup's row of partial sums: over the 8 groups of a wave (lanes l, l+8, ..), then over the waves in wave order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < BK_ACC; q++) {
        float v = acc[q];
        v += __shfl_xor(v, 8);
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (lane < BK_GROUP) s_red[(wave * BK_GROUP + lane) * BK_ACC + q] = v;
    }
    __syncthreads();
    float* out = partials + (size_t)blockIdx.x * BK_PARAMS;
    for (int t = threadIdx.x; t < BK_GROUP * BK_ACC; t += BK_THREADS) {
        const int ll = t / BK_ACC, q = t % BK_ACC;
        float v = 0.f;
        for (int wv = 0; wv < BK_THREADS / 64; wv++) v += s_red[(wv * BK_GROUP + ll) * BK_ACC + q];
        if (q < 16) out[16 * ll + q] = v;                              // dW1[4 ll + q / 4][q % 4]
        else if (q < 20) out[128 + 4 * ll + (q - 16)] = v;             // db1[4 ll + ..]
        else if (q < 32) out[160 + 32 * ((q - 20) / 4) + 4 * ll + (q - 20) % 4] = v;     // dW2[c][4 ll + ..]
        else if (ll == 0) out[256 + (q - 32)] = v;                     // db2: every lane of a group held the same dz
    }
}

// grads[p] = sum over the rows of partials[rows][259]: a wave per parameter; lane s adds rows s, s + 64, .. (at most BK_BWD_MAX_BLOCKS / 64,
// all requested at once), then the 64 sums are added as a fixed tree.
__global__ void __launch_bounds__(256) k_bank_fold(int rows, const float* __restrict__ partials, float* __restrict__ grads) {
    const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= BK_PARAMS) return;                                        // (a whole wave)
    float part[BK_BWD_MAX_BLOCKS / 64];
#pragma unroll
    for (int q = 0; q < BK_BWD_MAX_BLOCKS / 64; q++) {
        const int r = lane + 64 * q;
        part[q] = r < rows ? partials[(size_t)r * BK_PARAMS + p] : 0.f;
    }
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < BK_BWD_MAX_BLOCKS / 64; q++) v += part[q];
#pragma unroll
    for (int step = 1; step < 64; step *= 2) v += __shfl_xor(v, step);
    if (lane == 0) grads[p] = v;
}

struct AppHeads { const float* W1[2]; const float* b1[2]; const float* e[2]; const float* dW1[2]; const float* db1[2]; float* de[2]; };

// W1_out [2][32][din] | b1_out [2][32]: a thread per element
__global__ void __launch_bounds__(256) k_appearance_fold(int din, int A, AppHeads hd, float* __restrict__ W1_out, float* __restrict__ b1_out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int packed = 2 * 32 * din, full = din + A;
    if (t < packed) {
        const int h = t / (32 * din), u = (t % (32 * din)) / din, q = t % din;
        W1_out[t] = hd.W1[h][u * full + q];
    } else if (t < packed + 64) {
        const int h = (t - packed) / 32, u = (t - packed) % 32;
        const float* w = hd.W1[h] + u * full + din;
        float acc = hd.b1[h][u];
        for (int a = 0; a < A; a++) acc += w[a] * hd.e[h][a];
        b1_out[32 * h + u] = acc;
    }
}

// dW1_full [2][32][din + A] | de_color [A] | de_raydrop [A]: a thread per element
__global__ void __launch_bounds__(256) k_appearance_backward(int din, int A, AppHeads hd, float* __restrict__ dW1_full) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int full = din + A, wide = 2 * 32 * full;
    if (t < wide) {
        const int h = t / (32 * full), u = (t % (32 * full)) / full, q = t % full;
        dW1_full[t] = q < din ? hd.dW1[h][u * din + q] : hd.db1[h][u] * hd.e[h][q - din];
    } else if (t < wide + 2 * A) {
        const int h = (t - wide) / A, a = (t - wide) % A;
        float acc = 0.f;
        for (int u = 0; u < 32; u++) acc += hd.W1[h][u * full + din + a] * hd.db1[h][u];
        hd.de[h][a] = acc;
    }
}

int bank_backward_rows(int N) {
    const int rounds = (N + BK_ANCHORS - 1) / BK_ANCHORS;
    return rounds < 1 ? 1 : (rounds > BK_BWD_MAX_BLOCKS ? BK_BWD_MAX_BLOCKS : rounds);
}

}  // namespace

extern "C" {

int lidargs_ng_options_abi_version(void) { return LIDARGS_NG_OPTIONS_ABI_VERSION; }
const char* lidargs_ng_options_last_error(void) { return g_err; }

int lidargs_ng_bank_forward(int N, const uint8_t* visible_mask, const float* anchor_feat, const float* anchor, const float* cam_center,
                            const float* W1, const float* b1, const float* W2, const float* b2, float* feat_out, void* stream) {
    if (N < 0) return fail(LIDARGS_NG_OPTIONS_ERR_INVALID_ARGUMENT, "ng_bank_forward", "bad sizes");
    if (!cam_center || !W1 || !b1 || !W2 || !b2) return fail(LIDARGS_NG_OPTIONS_ERR_INVALID_ARGUMENT, "ng_bank_forward", "NULL pointer");
    if (N == 0) return 0;
    if (!anchor_feat || !anchor || !feat_out) return fail(LIDARGS_NG_OPTIONS_ERR_INVALID_ARGUMENT, "ng_bank_forward", "NULL pointer");
    const int rounds = (N + BK_ANCHORS - 1) / BK_ANCHORS;
    const float3 cam = make_float3(cam_center[0], cam_center[1], cam_center[2]);
    hipLaunchKernelGGL(k_bank_forward, dim3(rounds < BK_FWD_MAX_BLOCKS ? rounds : BK_FWD_MAX_BLOCKS), dim3(BK_THREADS), 0, (hipStream_t)stream,
                       N, visible_mask, anchor_feat, anchor, cam, W1, b1, W2, b2, feat_out);
    return launched(LIDARGS_NG_OPTIONS_ERR_HIP, "ng_bank_forward");
}

size_t lidargs_ng_bank_backward_partial_floats(int N) { return (size_t)bank_backward_rows(N < 0 ? 0 : N) * BK_PARAMS; }

int lidargs_ng_bank_backward(int N, const uint8_t* visible_mask, const float* anchor_feat, const float* anchor, const float* cam_center,
                             const float* W1, const float* b1, const float* W2, const float* b2, const float* dL_dfeat_out,
                             float* dL_danchor_feat, float* dL_danchor, float* dL_dparams, float* partials, size_t partial_floats,
                             void* stream) {
    if (N < 0) return fail(LIDARGS_NG_OPTIONS_ERR_INVALID_ARGUMENT, "ng_bank_backward", "bad sizes");
    if (!cam_center || !W1 || !b1 || !W2 || !b2) return fail(LIDARGS_NG_OPTIONS_ERR_INVALID_ARGUMENT, "ng_bank_backward", "NULL pointer");
    if (N == 0) return 0;
    if (!anchor_feat || !anchor || !dL_dfeat_out || !dL_danchor_feat || !dL_danchor || !dL_dparams || !partials)
        return fail(LIDARGS_NG_OPTIONS_ERR_INVALID_ARGUMENT, "ng_bank_backward", "NULL pointer");
    if (partial_floats < lidargs_ng_bank_backward_partial_floats(N)) return fail(LIDARGS_NG_OPTIONS_ERR_INVALID_ARGUMENT, "ng_bank_backward", "partials too small");
    const int rows = bank_backward_rows(N);
    const float3 cam = make_float3(cam_center[0], cam_center[1], cam_center[2]);
    hipLaunchKernelGGL(k_bank_backward, dim3(rows), dim3(BK_THREADS), 0, (hipStream_t)stream, N, visible_mask, anchor_feat, anchor, cam,
                       W1, b1, W2, b2, dL_dfeat_out, dL_danchor_feat, dL_danchor, partials);
    hipLaunchKernelGGL(k_bank_fold, dim3((BK_PARAMS + 3) / 4), dim3(256), 0, (hipStream_t)stream, rows, partials, dL_dparams);
    return launched(LIDARGS_NG_OPTIONS_ERR_HIP, "ng_bank_backward");
}

int lidargs_ng_appearance_fold(int din, int A, const float* W1_color, const float* b1_color, const float* e_color, const float* W1_raydrop,
                               const float* b1_raydrop, const float* e_raydrop, float* W1_out, float* b1_out, void* stream) {
    if ((din != 35 && din != 36) || A < 1 || A > (1 << 20)) return fail(LIDARGS_NG_OPTIONS_ERR_INVALID_ARGUMENT, "ng_appearance_fold", "bad sizes");
    if (!W1_color || !b1_color || !e_color || !W1_raydrop || !b1_raydrop || !e_raydrop || !W1_out || !b1_out)
        return fail(LIDARGS_NG_OPTIONS_ERR_INVALID_ARGUMENT, "ng_appearance_fold", "NULL pointer");
    AppHeads hd = {};
    hd.W1[0] = W1_color; hd.W1[1] = W1_raydrop; hd.b1[0] = b1_color; hd.b1[1] = b1_raydrop; hd.e[0] = e_color; hd.e[1] = e_raydrop;
    const int threads = 2 * 32 * din + 64;
    hipLaunchKernelGGL(k_appearance_fold, dim3((threads + 255) / 256), dim3(256), 0, (hipStream_t)stream, din, A, hd, W1_out, b1_out);
    return launched(LIDARGS_NG_OPTIONS_ERR_HIP, "ng_appearance_fold");
}

int lidargs_ng_appearance_backward(int din, int A, const float* W1_color, const float* e_color, const float* W1_raydrop,
                                   const float* e_raydrop, const float* dW1_main_color, const float* db1_color,
                                   const float* dW1_main_raydrop, const float* db1_raydrop, float* dW1_full, float* de_color,
                                   float* de_raydrop, void* stream) {
    if ((din != 35 && din != 36) || A < 1 || A > (1 << 20)) return fail(LIDARGS_NG_OPTIONS_ERR_INVALID_ARGUMENT, "ng_appearance_backward", "bad sizes");
    if (!W1_color || !e_color || !W1_raydrop || !e_raydrop || !dW1_main_color || !db1_color || !dW1_main_raydrop || !db1_raydrop ||
        !dW1_full || !de_color || !de_raydrop)
        return fail(LIDARGS_NG_OPTIONS_ERR_INVALID_ARGUMENT, "ng_appearance_backward", "NULL pointer");
    AppHeads hd = {};
    hd.W1[0] = W1_color; hd.W1[1] = W1_raydrop; hd.e[0] = e_color; hd.e[1] = e_raydrop;
    hd.dW1[0] = dW1_main_color; hd.dW1[1] = dW1_main_raydrop; hd.db1[0] = db1_color; hd.db1[1] = db1_raydrop;
    hd.de[0] = de_color; hd.de[1] = de_raydrop;
    const long long threads = 2LL * 32 * (din + A) + 2LL * A;
    hipLaunchKernelGGL(k_appearance_backward, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, din, A, hd, dW1_full);
    return launched(LIDARGS_NG_OPTIONS_ERR_HIP, "ng_appearance_backward");
}

}  // extern "C"
