// neural_gaussians_t16.inc -- the anchor decode's backward on 16x16x4 f32 tiles (included by neural_gaussians.hip, namespace lg).
//
// k_ng_backward_mfma (32x32x2 tiles, one wave of 64 anchors per SIMD, weights read from L1) keeps the matrix pipe busy for a third of
// its time (round 4: 885 us of a 1780-us training step at 667 k anchors x 6): the k-output heads are padded to 32 columns, the input's
// four narrow columns cost a whole tile, 240 accumulator registers and 40 KB of LDS per wave leave one wave per SIMD, and nothing hides
// the L1 round trip in front of every batch of products.  Here (k <= 6):
//   * a wave owns 32 anchors as two 16-row tiles; v_mfma_f32_16x16x4_f32 (exact f32, 32 cycles): the heads take one 16-column tile, the
//     covariance head three, the input gradient three (36 -> 48) -- 788 instructions of 2048 flops per 32 anchors against 1064 of 4096
//     per 64;
//   * the weight-gradient accumulators are 38 tiles of 4 registers (152 with the input gradient's six) instead of 15 of 16: two waves
//     per SIMD, eight per workgroup = one workgroup per CU;
//   * the workgroup stages all four MLPs' weights in LDS once (30 KB): every B operand is an LDS read;
//   * the sums over anchors (G1 = D1^T [X 1], G2 = D2^T H) take their D1 / H operands straight from the accumulator registers: the
//     reduction index is permuted (step s of row tile r covers anchors 16 r + 4 g + s, g = lane / 16 -- exactly element s of a C tile),
//     so H and D1 pass through LDS once (for the products that need them as A operands), not twice;
//   * the output-layer bias sums are column sums of the delta2 rows already in LDS (one lane per output column), not 60 wave reductions;
//   * the eight waves fold their accumulators through LDS in wave order (deterministic) into ONE partial row per workgroup: 256 rows of
//     41 KB for the reduction behind instead of 1024.
// Reference: gaussian_renderer/__init__.py:17-119 (the forward whose VJP this is); arithmetic as k_ng_backward / k_ng_backward_mfma.
typedef float ng_f4v __attribute__((ext_vector_type(4)));
typedef uint32_t ngt_u3 __attribute__((ext_vector_type(3), aligned(4)));
typedef uint32_t ngt_u2 __attribute__((ext_vector_type(2), aligned(4)));
#define NGT_LS 33                                   // row stride of the per-wave [unit][anchor] arrays (32 anchors)
#define NGT_WS 41                                   // row stride of the first-layer weights [m][t][q]: q < din, zeros behind
#define NGT_WAVES 8
#define NGT_D2R(K) ((7 * (K) + 3) / 4 * 4)          // rows of y / delta2, whole 4-row steps
#define NGT_WAVE_FLOATS(K) ((40 + 32 + NGT_D2R(K)) * NGT_LS + 32)
#define NGT_W2ROWS(K) (10 * (K) + 4)
#define NGT_WEIGHT_FLOATS(K) (128 * NGT_WS + 128 + NGT_W2ROWS(K) * NGT_LS + 64)

__device__ __forceinline__ ng_f4v ngt_mfma(float a, float b, ng_f4v c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ ng_f4v ngt_splat(float v) { ng_f4v c; c[0] = v; c[1] = v; c[2] = v; c[3] = v; return c; }

#define NGT_FENCE() __builtin_amdgcn_sched_barrier(0)

// A load under a per-lane condition compiles to a branch around it and a full wait at the join -- nine conditional gathers are nine
// round trips one after the other (ISA of the first form; ~5 k cycles each, tools/t16_where.sh).  So every per-lane load of these
// kernels is UNCONDITIONAL from an index any lane may read (its own when it has one, otherwise a neighbour's), and what a lane has no
// use for is dropped by a select afterwards.  ngt_row: the lane's selected row, or the first selected lane's of the wave.
__device__ __forceinline__ uint32_t ngt_row(bool sel, uint32_t r, unsigned long long any) {
    const uint32_t rf = (uint32_t)__builtin_amdgcn_readlane((int)r, __ffsll((long long)any) - 1);
    return sel ? r : rf;
}
#ifdef LG_NG_T16_DIAG       // clock stamps per part of the tile (tools/t16_where.sh): a wave's cycles between the marks, printed by a few waves
#define NGT_TICK(k) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); tk[k] += t_ - tlast; tlast = t_; } while (0)
#else
#define NGT_TICK(k) do { } while (0)
#endif   // operand loads stay in front of the products they feed (in-order LDS returns pipeline the rest)

// One MLP of the tile, first half: h = relu(X W1^T + b1) -> s_t (transposed: the A operand of the second layer, and the mask / B operand
// the back-propagation reads back) and y = H W2^T + b2 -> s_d2 rows [0, DOUT).  All operands of a product are requested before its
// first instruction: with two waves per SIMD the other wave's products run while they arrive.
template <int MM, int DOUT, int OBASE>
__device__ __forceinline__ void ngt_recompute(const float* __restrict__ sW1, const float* __restrict__ sb1, const float* __restrict__ sW2,
                                              const float* __restrict__ sb2, const float* __restrict__ s_x, float* __restrict__ s_t,
                                              float* __restrict__ s_d2, int lane) {
    const int c = lane & 15, g = lane >> 4;
    {
        const float* ax = s_x + g * NGT_LS + c;                        // A[i = anchor c (+16 r)][k = q = 4 s + g]
        const float* bw = sW1 + (MM * 32 + c) * NGT_WS + g;            // B[k = q][j = t = c (+16 tc)] = W1[t][q]
        float a0[9], a1[9], b0[9], b1[9];
#pragma unroll
        for (int s = 0; s < 9; s++) { a0[s] = ax[4 * s * NGT_LS]; a1[s] = ax[4 * s * NGT_LS + 16]; b0[s] = bw[4 * s]; b1[s] = bw[16 * NGT_WS + 4 * s]; }
        const float bias0 = sb1[MM * 32 + c], bias1 = sb1[MM * 32 + 16 + c];
        NGT_FENCE();
        ng_f4v h00 = ngt_splat(bias0), h10 = h00, h01 = ngt_splat(bias1), h11 = h01;
#pragma unroll
        for (int s = 0; s < 9; s++) {
            h00 = ngt_mfma(a0[s], b0[s], h00); h10 = ngt_mfma(a1[s], b0[s], h10);
            h01 = ngt_mfma(a0[s], b1[s], h01); h11 = ngt_mfma(a1[s], b1[s], h11);
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
            s_t[c * NGT_LS + 4 * g + e] = fmaxf(h00[e], 0.f); s_t[c * NGT_LS + 16 + 4 * g + e] = fmaxf(h10[e], 0.f);
            s_t[(16 + c) * NGT_LS + 4 * g + e] = fmaxf(h01[e], 0.f); s_t[(16 + c) * NGT_LS + 16 + 4 * g + e] = fmaxf(h11[e], 0.f);
        }
    }
    __builtin_amdgcn_wave_barrier();
    constexpr int OC = (DOUT + 15) / 16;
    const float* at = s_t + g * NGT_LS + c;                            // A[i = anchor][k = t = 4 s + g]
    float a0[8], a1[8];
#pragma unroll
    for (int s = 0; s < 8; s++) { a0[s] = at[4 * s * NGT_LS]; a1[s] = at[4 * s * NGT_LS + 16]; }
#pragma unroll
    for (int oc = 0; oc < OC; oc++) {
        const int o = 16 * oc + c, oe = o < DOUT ? o : DOUT - 1;
        const float* bw2 = sW2 + (OBASE + oe) * NGT_LS + g;            // B[k = t][j = o] = W2[o][t]
        float b[8];
#pragma unroll
        for (int s = 0; s < 8; s++) b[s] = bw2[4 * s];
        ng_f4v y0 = ngt_splat(sb2[OBASE + oe]), y1 = y0;
        NGT_FENCE();
#pragma unroll
        for (int s = 0; s < 8; s++) { y0 = ngt_mfma(a0[s], b[s], y0); y1 = ngt_mfma(a1[s], b[s], y1); }
        if (o < DOUT) {
#pragma unroll
            for (int e = 0; e < 4; e++) { s_d2[o * NGT_LS + 4 * g + e] = y0[e]; s_d2[o * NGT_LS + 16 + 4 * g + e] = y1[e]; }
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// Second half (delta2 is in s_d2, its rows DOUT .. 4 ceil(DOUT / 4) - 1 are zero; h is in s_t): D1 = (D2 W2) * relu'(h); the two sums
// over the anchors; dX += D1 W1.  g1m: this MLP's G1 columns 0..31 as [t tile][q tile]; g1n: columns 32..39 of the MLP pair MM / 2 (MM
// owns columns 8 (MM & 1) ..); g2: [o tile][t tile].
template <int MM, int DOUT, int OBASE, int D2ROWS>
__device__ __forceinline__ void ngt_backprop(const float* __restrict__ sW1, const float* __restrict__ sW2, const float* __restrict__ s_x,
                                             float* __restrict__ s_t, const float* __restrict__ s_d2, int lane,
                                             ng_f4v (&dx)[2][3], ng_f4v (&g1m)[2][2], ng_f4v (&g1n)[2], ng_f4v (&g2)[(DOUT + 15) / 16][2]) {
    constexpr int OR = (DOUT + 15) / 16, KS = (DOUT + 3) / 4, KB = 6;      // KB: steps of D2 W2 whose operands are requested together
    const int c = lane & 15, g = lane >> 4;
    ng_f4v d1[2][2];
    {
        const float* ad = s_d2 + g * NGT_LS + c;                       // A[i = anchor][k = o = 4 s + g]
        const float* bw = sW2 + (OBASE + g) * NGT_LS + c;              // B[k = o][j = t]
        d1[0][0] = ngt_splat(0.f); d1[0][1] = d1[0][0]; d1[1][0] = d1[0][0]; d1[1][1] = d1[0][0];
#pragma unroll
        for (int s0 = 0; s0 < KS; s0 += KB) {
            float a0[KB], a1[KB], b0[KB], b1[KB];
#pragma unroll
            for (int q = 0; q < KB; q++) if (s0 + q < KS) {
                const int s = s0 + q;
                a0[q] = ad[4 * s * NGT_LS]; a1[q] = ad[4 * s * NGT_LS + 16]; b0[q] = bw[4 * s * NGT_LS]; b1[q] = bw[4 * s * NGT_LS + 16];
            }
            NGT_FENCE();
#pragma unroll
            for (int q = 0; q < KB; q++) if (s0 + q < KS) {
                d1[0][0] = ngt_mfma(a0[q], b0[q], d1[0][0]); d1[1][0] = ngt_mfma(a1[q], b0[q], d1[1][0]);
                d1[0][1] = ngt_mfma(a0[q], b1[q], d1[0][1]); d1[1][1] = ngt_mfma(a1[q], b1[q], d1[1][1]);
            }
        }
    }
    // sums over the anchors: step (r, s) covers anchors 16 r + 4 g + s = element s of the C tiles of row tile r; h comes back from s_t in
    // that layout (relu' and the B operand of G2)
    {
        const bool mine = (c >> 3) == (MM & 1);
        const float* xb = s_x + c * NGT_LS + 4 * g;                    // B[k = anchor][j = q = c (+16)] = X[anchor][q]
        const float* xn = s_x + (32 + (c & 7)) * NGT_LS + 4 * g;       // narrow columns 32..39 (36 = the constant 1: the bias gradient)
        const float* hb = s_t + c * NGT_LS + 4 * g;                    // H[anchor][t = c (+16)]
        int orow[OR];
#pragma unroll
        for (int q = 0; q < OR; q++) { const int o = 16 * q + c; orow[q] = (o < D2ROWS ? o : D2ROWS - 1) * NGT_LS + 4 * g; }
#pragma unroll
        for (int r = 0; r < 2; r++) {
            float b0[4], b1[4], bn[4], h0[4], h1[4], a2[OR][4];
#pragma unroll
            for (int s = 0; s < 4; s++) {
                b0[s] = xb[16 * r + s]; b1[s] = xb[16 * NGT_LS + 16 * r + s]; bn[s] = xn[16 * r + s];
                h0[s] = hb[16 * r + s]; h1[s] = hb[16 * NGT_LS + 16 * r + s];
#pragma unroll
                for (int q = 0; q < OR; q++) a2[q][s] = s_d2[orow[q] + 16 * r + s];      // A[i = o][k = anchor]
            }
            NGT_FENCE();
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const float bnm = mine ? bn[s] : 0.f;
                d1[r][0][s] = h0[s] > 0.f ? d1[r][0][s] : 0.f;
                d1[r][1][s] = h1[s] > 0.f ? d1[r][1][s] : 0.f;
#pragma unroll
                for (int tr = 0; tr < 2; tr++) {
                    const float a = d1[r][tr][s];                                          // A[i = t][k = anchor]
                    g1m[tr][0] = ngt_mfma(a, b0[s], g1m[tr][0]);
                    g1m[tr][1] = ngt_mfma(a, b1[s], g1m[tr][1]);
                    g1n[tr] = ngt_mfma(a, bnm, g1n[tr]);
                }
#pragma unroll
                for (int q = 0; q < OR; q++) {
                    g2[q][0] = ngt_mfma(a2[q][s], h0[s], g2[q][0]);                        // B[k = anchor][j = t] = H
                    g2[q][1] = ngt_mfma(a2[q][s], h1[s], g2[q][1]);
                }
            }
        }
    }
    __builtin_amdgcn_wave_barrier();                                   // h's copy in s_t is dead now: D1 takes its place
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int tc = 0; tc < 2; tc++)
#pragma unroll
            for (int e = 0; e < 4; e++) s_t[(16 * tc + c) * NGT_LS + 16 * r + 4 * g + e] = d1[r][tc][e];
    __builtin_amdgcn_wave_barrier();
    {
        const float* at = s_t + g * NGT_LS + c;                        // A[i = anchor][k = t = 4 s + g] = D1
        const float* bw = sW1 + (MM * 32 + g) * NGT_WS + c;            // B[k = t][j = q] = W1[t][q]
        const float* bwn = sW1 + (MM * 32 + g) * NGT_WS + 32 + (c & 7);
        float a0[8], a1[8], b0[8], b1[8], b2[8];
#pragma unroll
        for (int s = 0; s < 8; s++) {
            a0[s] = at[4 * s * NGT_LS]; a1[s] = at[4 * s * NGT_LS + 16];
            b0[s] = bw[4 * s * NGT_WS]; b1[s] = bw[4 * s * NGT_WS + 16]; b2[s] = bwn[4 * s * NGT_WS];
        }
        NGT_FENCE();
#pragma unroll
        for (int s = 0; s < 8; s++) {
            dx[0][0] = ngt_mfma(a0[s], b0[s], dx[0][0]); dx[1][0] = ngt_mfma(a1[s], b0[s], dx[1][0]);
            dx[0][1] = ngt_mfma(a0[s], b1[s], dx[0][1]); dx[1][1] = ngt_mfma(a1[s], b1[s], dx[1][1]);
            dx[0][2] = ngt_mfma(a0[s], b2[s], dx[0][2]); dx[1][2] = ngt_mfma(a1[s], b2[s], dx[1][2]);
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// column sums of the delta2 rows (one lane per output column; lanes [lane0, lane0 + DOUT) own this MLP's columns)
template <int DOUT>
__device__ __forceinline__ float ngt_bias_sums(const float* __restrict__ s_d2, int lane, int lane0) {
    float acc = 0.f;
    const int row = lane - lane0;
    if (row >= 0 && row < DOUT) {
        const float* p = s_d2 + row * NGT_LS;
#pragma unroll
        for (int a0 = 0; a0 < 32; a0 += 16) {                          // sixteen reads in flight, then their sum in order
            float v[16];
#pragma unroll
            for (int q = 0; q < 16; q++) v[q] = p[a0 + q];
            NGT_FENCE();
#pragma unroll
            for (int q = 0; q < 16; q++) acc += v[q];
        }
    }
    return acc;
}

// the per-anchor stage of one of the three k-output MLPs: lane = (anchor a, half hh); half hh takes the offsets j = hh JH + jj, JH = (k + 1) / 2
// (consecutive offsets: their words are neighbours in memory); slj[jj]: output row of (anchor, offset hh JH + jj), ~0 = not selected (fetched at the top of the tile)
template <int K, int WHICH>
__device__ __forceinline__ void ngt_small_fetch_cond(bool active, size_t cidx, int hh, const uint32_t (&slj)[(K + 1) / 2], const float* __restrict__ g_opacity,
                                                     const float* __restrict__ g_color, const float* __restrict__ g_no, float (&gg)[(K + 1) / 2]) {
#pragma unroll
    for (int jj = 0; jj < (K + 1) / 2; jj++) {                        // (the first form: a load per selected lane under its own condition)
        const int j = hh * ((K + 1) / 2) + jj;
        const uint32_t r = slj[jj];
        gg[jj] = 0.f;
        if (r != 0xFFFFFFFFu) gg[jj] = WHICH == 0 ? g_opacity[r] : (WHICH == 1 ? g_color[2 * (size_t)r] : g_color[2 * (size_t)r + 1]);
        if (WHICH == 0 && g_no && active && j < K) gg[jj] += g_no[cidx * K + j];
    }
}
template <int K, int WHICH>
__device__ __forceinline__ void ngt_small_fetch(bool active, size_t cidx, int hh, const uint32_t (&slj)[(K + 1) / 2], const float* __restrict__ g_opacity,
                                                const float* __restrict__ g_color, const float* __restrict__ g_no, float (&gg)[(K + 1) / 2]) {
    constexpr int JH = (K + 1) / 2;
#pragma unroll
    for (int jj = 0; jj < JH; jj++) {                                 // requested in front of the MLP's recompute, used behind it
        const int j = hh * JH + jj, jc = j < K ? j : K - 1;
        const bool sel = slj[jj] != 0xFFFFFFFFu;
        const unsigned long long any = __ballot(sel);
        float v = 0.f;
        if (any) {                                                     // (wave-uniform)
            const uint32_t r = ngt_row(sel, slj[jj], any);
            v = WHICH == 0 ? g_opacity[r] : (WHICH == 1 ? g_color[2 * (size_t)r] : g_color[2 * (size_t)r + 1]);
        }
        gg[jj] = sel ? v : 0.f;
        if (WHICH == 0 && g_no) {                                      // (visible anchors only are active: cidx is a row of g_no's)
            const float w = g_no[(active ? cidx : 0) * K + jc];
            if (active && j < K) gg[jj] += w;
        }
    }
}
template <int K, int WHICH>
__device__ __forceinline__ void ngt_small_deltas(bool active, int a, int hh, const float (&gg)[(K + 1) / 2], float* __restrict__ s_d2) {
    constexpr int KP = (K + 3) / 4 * 4, JH = (K + 1) / 2;
#pragma unroll
    for (int jj = 0; jj < JH; jj++) {
        const int j = hh * JH + jj;
        if (j < K) {
            float d = 0.f;
            if (active) d = ng_head_delta<WHICH>(s_d2[j * NGT_LS + a], gg[jj]);
            s_d2[j * NGT_LS + a] = d;
        }
    }
    if (hh == 0) {
#pragma unroll
        for (int j = K; j < KP; j++) s_d2[j * NGT_LS + a] = 0.f;       // the products step through 4 rows
    }
}

// The four MLPs' weights into LDS: sW1 [m][t][NGT_WS] (q < din, zeros behind: a 35-input MLP ignores the distance), sb1 [m][t], sW2 rows
// [k | 7k | k | k] = opacity, covariance, colour, ray-drop (+4 zero rows: the products step through 4), sb2 likewise.
template <int K, int NT, int MLPS = 15>                            // MLPS: bit m set = MLP m is staged (a launch stages what it multiplies with)
__device__ __forceinline__ void ngt_stage_weights(const NgModel& m, float* __restrict__ sW1, float* __restrict__ sb1, float* __restrict__ sW2,
                                                  float* __restrict__ sb2, int tid) {
    // every load of every staged MLP is requested before the first LDS store (a loop of load -> store pays a round trip per trip: the
    // first form took ~8 us of every launch to stage 30 KB)
    constexpr int C1 = (32 * NGT_WS + NT - 1) / NT, C2 = (7 * K * NGT_LS + NT - 1) / NT;
    float v1[4][C1], v2[4][C2], vb1[4], vb2[4];
#pragma unroll
    for (int mm = 0; mm < 4; mm++) {
        const bool on = ((MLPS >> mm) & 1) != 0;
        const int dout = ng_dout(mm, K);
        const int din = on ? m.din[mm] : 36;
        const float* __restrict__ W1 = m.W1[mm];
        const float* __restrict__ W2 = m.W2[mm];
#pragma unroll
        for (int it = 0; it < C1; it++) {
            const int q = tid + it * NT, t = q / NGT_WS, col = q - t * NGT_WS;
            v1[mm][it] = 0.f;
            if (on) {                                                  // (compile-time; the load itself is unconditional: see ngt_row)
                const bool in = q < 32 * NGT_WS && col < din;
                const float w = W1[in ? t * din + col : 0];
                v1[mm][it] = in ? w : 0.f;
            }
        }
#pragma unroll
        for (int it = 0; it < C2; it++) {
            const int q = tid + it * NT, o = q / NGT_LS, col = q - o * NGT_LS;
            v2[mm][it] = 0.f;
            if (on) {
                const bool in = q < dout * NGT_LS && col < 32;
                const float w = W2[in ? o * 32 + col : 0];
                v2[mm][it] = in ? w : 0.f;
            }
        }
        vb1[mm] = 0.f; vb2[mm] = 0.f;
        if (on) {
            const float x1 = m.b1[mm][tid < 32 ? tid : 0], x2 = m.b2[mm][tid < dout ? tid : 0];
            vb1[mm] = tid < 32 ? x1 : 0.f; vb2[mm] = tid < dout ? x2 : 0.f;
        }
    }
#pragma unroll
    for (int mm = 0; mm < 4; mm++) {                                   // (zeros where nothing is staged: a product's padding steps may run into a
        const int dout = ng_dout(mm, K), obase = ng_col0(mm, K);   //  neighbour's rows -- times zero: they must be finite)
#pragma unroll
        for (int it = 0; it < C1; it++) { const int q = tid + it * NT; if (q < 32 * NGT_WS) sW1[mm * 32 * NGT_WS + q] = v1[mm][it]; }
#pragma unroll
        for (int it = 0; it < C2; it++) { const int q = tid + it * NT; if (q < dout * NGT_LS) sW2[obase * NGT_LS + q] = v2[mm][it]; }
        if (tid < 32) sb1[mm * 32 + tid] = vb1[mm];
        if (tid < dout) sb2[obase + tid] = vb2[mm];
    }
    for (int q = tid; q < 4 * NGT_LS; q += NT) sW2[10 * K * NGT_LS + q] = 0.f;       // the zero rows behind the last MLP's
}

// PASS 0: the four MLPs in one launch; 1: the covariance MLP (and the direct paths of xyz / scaling);
// 2: the opacity / colour / ray-drop MLPs (and the zero rows of anchors without work: `PASS != 1`).  2 is launched first; 1 adds its share to the rows 2 stored (requested at the top of the tile).  One launch holds 152 accumulator registers for
// the life of the wave and the compiler spills whatever else a tile touches (addresses, the words loaded at the top of a tile, one by
// one with a wait each): two launches hold 72 and 112.
template <int K, int PASS>
__global__ void __launch_bounds__(64 * NGT_WAVES) k_ng_backward_t16(int N, NgModel m, float3 cam, const float* __restrict__ feat, const float* __restrict__ anchor,
                                                                    const float* __restrict__ offset, const float* __restrict__ scaling,
                                                                    const uint32_t* __restrict__ vis_flags, const uint32_t* __restrict__ vis_idx,
                                                                    const uint32_t* __restrict__ sel_flags, const uint32_t* __restrict__ slot,
                                                                    const float* __restrict__ g_xyz, const float* __restrict__ g_color, const float* __restrict__ g_opacity,
                                                                    const float* __restrict__ g_scaling, const float* __restrict__ g_rot, const float* __restrict__ g_no,
                                                                    float* __restrict__ d_feat, float* __restrict__ d_anchor, float* __restrict__ d_offset,
                                                                    float* __restrict__ d_scaling, float* __restrict__ partial, int stagger) {
    static_assert(10 * K <= 64, "one lane per output column");
    constexpr int NC = NG_COV_TILES(K), D2R = NGT_D2R(K), PER = ng_partial_floats(K);
    constexpr int ORC = (7 * K + 15) / 16;
    constexpr int C_OPA = ng_col0(NG_OPA, K), C_COV = ng_col0(NG_COV, K), C_COL = ng_col0(NG_COL, K), C_RD = ng_col0(NG_RD, K);
    static_assert(16 * ORC <= 32 * NC, "the covariance head's G2 tiles fit its blocks of the partial row");
    static_assert(NGT_WAVES * NGT_WAVE_FLOATS(K) >= PER, "the fold reuses the waves' arrays");
    __shared__ float s_all[NGT_WEIGHT_FLOATS(K) + NGT_WAVES * NGT_WAVE_FLOATS(K)];
    float* const sW1 = s_all;
    float* const sb1 = sW1 + 128 * NGT_WS;
    float* const sW2 = sb1 + 128;
    float* const sb2 = sW2 + NGT_W2ROWS(K) * NGT_LS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* const s_x = s_all + NGT_WEIGHT_FLOATS(K) + wave * NGT_WAVE_FLOATS(K);
    float* const s_t = s_x + 40 * NGT_LS;
    float* const s_d2 = s_t + 32 * NGT_LS;
    uint32_t* const s_act = reinterpret_cast<uint32_t*>(s_d2 + D2R * NGT_LS);
    ngt_stage_weights<K, 64 * NGT_WAVES, (PASS == 1 ? 2 : (PASS == 2 ? 13 : 15))>(m, sW1, sb1, sW2, sb2, tid);     // once per workgroup: the MLPs this launch runs
    for (int q = lane; q < NGT_WAVE_FLOATS(K); q += 64) s_x[q] = 0.f;   // nothing a product can meet is ever uninitialised
    __syncthreads();

    ng_f4v g1[4][2][2], g1n[2][2], g2o[1][2], g2c[ORC][2], g2l[1][2], g2r[1][2];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) { g1[a][b][0] = ngt_splat(0.f); g1[a][b][1] = ngt_splat(0.f); }
#pragma unroll
    for (int b = 0; b < 2; b++) {
        g1n[0][b] = ngt_splat(0.f); g1n[1][b] = ngt_splat(0.f); g2o[0][b] = ngt_splat(0.f); g2l[0][b] = ngt_splat(0.f); g2r[0][b] = ngt_splat(0.f);
#pragma unroll
        for (int q = 0; q < ORC; q++) g2c[q][b] = ngt_splat(0.f);
    }
    float db2 = 0.f;                                                   // lane = output column: [k | 7k | k | k] = opacity, covariance, colour, ray-drop
    const int c16 = lane & 15, g4 = lane >> 4;
    const int a = lane & 31, hh = lane >> 5;
    const int ntiles = (N + 31) / 32;
    const int tstride = gridDim.x * NGT_WAVES;
    // start-up skew (LIDARGS_NG_T16_STAGGER, default 0 = none): the waves run identical tiles in lockstep, so the whole chip loads, computes
    // and stores at the same moments; wave w waits w x stagger x 8 k clocks before its first tile
    for (int q = 0; q < wave * stagger; q++) __builtin_amdgcn_s_sleep(127);
#ifdef LG_NG_T16_DIAG
    unsigned long long tk[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tlast = __builtin_amdgcn_s_memtime();
    int tiles_done = 0;
    const char* skp = nullptr; (void)skp;
#endif
    for (int tile = blockIdx.x * NGT_WAVES + wave; tile < ntiles; tile += tstride) {
        const int i = tile * 32 + a;
        // Everything the tile needs from memory before its first product in ONE round trip: the bookkeeping words (visible flag, compact
        // index, selection flags and output rows of the lane's offsets -- every array holds a word for every anchor / offset, so none
        // waits for another), the anchor position, and the 4 KB of features (four 1-KB wave loads; rows of anchors without work are read
        // too -- the flags are not here yet -- and dropped when the tile is staged).  The clock stamps of the first form
        // (tools/t16_where.sh) showed ~8 k cycles per dependent round trip and five of them per tile: half of the kernel's time.
        uint32_t nvis = 0u, ncidx = 0u, nsel[(K + 1) / 2], nslot[(K + 1) / 2];
        float nax = 0.f, nay = 0.f, naz = 0.f;
        float4 nf[4];
#pragma unroll
        for (int jj = 0; jj < (K + 1) / 2; jj++) { nsel[jj] = 0u; nslot[jj] = 0u; }
        float4 pf[4];                                                  // PASS 1: what the launch in front stored in this tile's rows of d_feat, d_anchor
        float3 pa = make_float3(0.f, 0.f, 0.f);
        if constexpr (PASS == 2) {
            // (the heads' launch keeps the first form, loads under the lanes' own conditions: with its 112 accumulator registers the
            //  unconditional form below measured 27 us slower -- A/B of the two sources in one run, tools/t16_variants.sh)
            if (i < N) {
                nvis = vis_flags[i]; ncidx = vis_idx[i];
                constexpr int JH = (K + 1) / 2;
                const size_t w0 = (size_t)i * K + hh * JH;             // this lane's offsets are neighbours: one load per array where k is even
                if (K == 6) {
                    const ngt_u3 f = *reinterpret_cast<const ngt_u3*>(sel_flags + w0), r = *reinterpret_cast<const ngt_u3*>(slot + w0);
                    nsel[0] = f.x; nsel[1] = f.y; nsel[JH - 1] = f.z; nslot[0] = r.x; nslot[1] = r.y; nslot[JH - 1] = r.z;
                } else if (K == 4) {
                    const ngt_u2 f = *reinterpret_cast<const ngt_u2*>(sel_flags + w0), r = *reinterpret_cast<const ngt_u2*>(slot + w0);
                    nsel[0] = f.x; nsel[1] = f.y; nslot[0] = r.x; nslot[1] = r.y;
                } else {
#pragma unroll
                    for (int jj = 0; jj < JH; jj++) if (hh * JH + jj < K) { nsel[jj] = sel_flags[w0 + jj]; nslot[jj] = slot[w0 + jj]; }
                }
                const float3 an = get3(anchor, (size_t)i);
                nax = an.x; nay = an.y; naz = an.z;
            }
            const float4* f4 = reinterpret_cast<const float4*>(feat) + (size_t)tile * (32 * NG_FEAT / 4);
#pragma unroll
            for (int it = 0; it < 4; it++) {
                const int idx = it * 64 + lane;
                nf[it] = make_float4(0.f, 0.f, 0.f, 0.f); pf[it] = nf[it];
                if (tile * 32 + (idx >> 3) < N) nf[it] = f4[idx];
            }
        } else {
        {
            constexpr int JH = (K + 1) / 2;
            const size_t ic = i < N ? i : N - 1;                       // (unconditional loads from a row every lane may read; dropped below)
            nvis = vis_flags[ic]; ncidx = vis_idx[ic];
            const size_t w0 = ic * K + hh * JH;                        // this lane's offsets are neighbours: one load per array where k is even
            if (K == 6) {
                const ngt_u3 f = *reinterpret_cast<const ngt_u3*>(sel_flags + w0), r = *reinterpret_cast<const ngt_u3*>(slot + w0);
                nsel[0] = f.x; nsel[1] = f.y; nsel[JH - 1] = f.z; nslot[0] = r.x; nslot[1] = r.y; nslot[JH - 1] = r.z;
            } else if (K == 4) {
                const ngt_u2 f = *reinterpret_cast<const ngt_u2*>(sel_flags + w0), r = *reinterpret_cast<const ngt_u2*>(slot + w0);
                nsel[0] = f.x; nsel[1] = f.y; nslot[0] = r.x; nslot[1] = r.y;
            } else {
#pragma unroll
                for (int jj = 0; jj < JH; jj++) {
                    const int j = hh * JH + jj, jc = j < K ? j : K - 1;
                    nsel[jj] = sel_flags[ic * K + jc]; nslot[jj] = slot[ic * K + jc];
                    if (j >= K) nsel[jj] = 0u;
                }
            }
            const float3 an = get3(anchor, ic);
            nax = an.x; nay = an.y; naz = an.z;
            if (i >= N) nvis = 0u;
        }
        {
            const float4* f4 = reinterpret_cast<const float4*>(feat);
            const float4* p4 = reinterpret_cast<const float4*>(d_feat);
#pragma unroll
            for (int it = 0; it < 4; it++) {
                const int idx = it * 64 + lane;
                const size_t ga = (size_t)tile * 32 + (idx >> 3);
                const size_t gi = (ga < (size_t)N ? ga : (size_t)N - 1) * (NG_FEAT / 4) + (idx & 7);     // (rows past the end: the last row's, never used)
                nf[it] = f4[gi];
                pf[it] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (PASS == 1) pf[it] = p4[gi];
            }
            if (PASS == 1) pa = get3(d_anchor, i < N ? (size_t)i : (size_t)N - 1);
        }
        }
        bool active = false;
        size_t cidx = 0;
        uint32_t slj[(K + 1) / 2];                                     // output rows of this lane's offsets (hh JH + jj), ~0 = not selected
        bool own = false;
#pragma unroll
        for (int jj = 0; jj < (K + 1) / 2; jj++) {
            const bool on = nvis != 0u && nsel[jj] != 0u;
            slj[jj] = on ? nslot[jj] : 0xFFFFFFFFu;
            own = own || on;
        }
        if (nvis) cidx = ncidx;
        {
            const int other = __shfl_xor((int)own, 32);               // the two halves of an anchor agree (no short circuit around the exchange)
            active = nvis != 0u && (own || other != 0 || g_no != nullptr);   // with a gradient on neural_opacity every visible anchor has work
        }
        if (i < N && PASS != 1) {
            const bool zero_dense = !active;
            if (zero_dense) {                                          // every row of the dense outputs is written (the halves share the row)
                if (hh == 0) {
                    float4* df = reinterpret_cast<float4*>(d_feat + (size_t)i * NG_FEAT);
#pragma unroll
                    for (int q = 0; q < NG_FEAT / 4; q++) df[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                } else {
                    float* dofs = d_offset + 3 * (size_t)i * K;
                    for (int q = 0; q < 3 * K; q++) dofs[q] = 0.f;
                    for (int q = 0; q < 3; q++) d_anchor[3 * (size_t)i + q] = 0.f;
                    for (int q = 0; q < 6; q++) d_scaling[6 * (size_t)i + q] = 0.f;
                }
            }
        }
        if (__ballot(active) == 0ull) continue;                        // nothing to fold in this tile
        NGT_TICK(0);
        __builtin_amdgcn_wave_barrier();
        if (hh == 0) s_act[a] = active ? 1u : 0u;
        __builtin_amdgcn_wave_barrier();
        {
#pragma unroll
            for (int it = 0; it < 4; it++) {
                const int idx = it * 64 + lane;
                const int aa = idx >> 3, qb = (idx & 7) * 4;
                float4 v = nf[it];
                if (!s_act[aa]) v = make_float4(0.f, 0.f, 0.f, 0.f);
                s_x[(qb + 0) * NGT_LS + aa] = v.x; s_x[(qb + 1) * NGT_LS + aa] = v.y; s_x[(qb + 2) * NGT_LS + aa] = v.z; s_x[(qb + 3) * NGT_LS + aa] = v.w;
            }
            if (hh == 0) {
                float4 vd = make_float4(0.f, 0.f, 0.f, 0.f);
                if (active) vd = ng_view(make_float3(nax, nay, naz), cam);
                s_x[32 * NGT_LS + a] = vd.x; s_x[33 * NGT_LS + a] = vd.y; s_x[34 * NGT_LS + a] = vd.z; s_x[35 * NGT_LS + a] = vd.w;
                s_x[36 * NGT_LS + a] = active ? 1.f : 0.f;             // the constant input: the first-layer bias gradients fall out of G1
            }
        }
        float da[3] = {0.f, 0.f, 0.f};
        ng_f4v dx[2][3];
#pragma unroll
        for (int r = 0; r < 2; r++) { dx[r][0] = ngt_splat(0.f); dx[r][1] = ngt_splat(0.f); dx[r][2] = ngt_splat(0.f); }
        __builtin_amdgcn_wave_barrier();

        NGT_TICK(1);
        if constexpr (PASS != 2) {
        // --- covariance MLP: scaling = s[3:6] * sigmoid(sr[0:3]), rot = normalize(sr[3:7]); and the direct paths of xyz / scaling
        // whole rows per instruction (4-byte-aligned vector types: 19 vector-memory instructions instead of 60).  In the launch of its own
        // the stage's rows are requested in front of the MLP's recompute (45 registers the single launch does not have) and arrive behind it.
        constexpr int JH = (K + 1) / 2;
        float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float3 gxyz[JH], gsc[JH], gof[JH];
        float4 grot[JH];
        auto cov_fetch = [&]() {
            const size_t ic = i < N ? i : N - 1;                       // (unconditional loads: see ngt_row)
            const row4 sa = *reinterpret_cast<const row4*>(scaling + 6 * ic);
            const row2 sb = *reinterpret_cast<const row2*>(scaling + 6 * ic + 4);
            s[0] = sa.x; s[1] = sa.y; s[2] = sa.z; s[3] = sa.w; s[4] = sb.x; s[5] = sb.y;
#pragma unroll
            for (int jj = 0; jj < JH; jj++) {
                const int j = hh * JH + jj, jc = j < K ? j : K - 1;
                const bool on = active && j < K, sel = on && slj[jj] != 0xFFFFFFFFu;
                const unsigned long long any = __ballot(sel);
                gxyz[jj] = make_float3(0.f, 0.f, 0.f); gsc[jj] = gxyz[jj];
                grot[jj] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (any) {                                             // (wave-uniform)
                    const size_t r = ngt_row(sel, slj[jj], any);
                    const float3 x = get3(g_xyz, r), sc = get3(g_scaling, r);
                    const float4 q = get4(g_rot, r);
                    if (sel) { gxyz[jj] = x; gsc[jj] = sc; grot[jj] = q; }
                }
                const float3 o = get3(offset, ic * K + jc);
                gof[jj] = on ? o : make_float3(0.f, 0.f, 0.f);
            }
        };
        if constexpr (PASS == 1) cov_fetch();
        ngt_recompute<NG_COV, 7 * K, C_COV>(sW1, sb1, sW2, sb2, s_x, s_t, s_d2, lane);
        NGT_TICK(2);
        if constexpr (PASS != 1) cov_fetch();
        {
            float ds[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            float3 dof[JH];
#pragma unroll
            for (int jj = 0; jj < JH; jj++) {
                const int j = hh * JH + jj;
                float d[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                dof[jj] = make_float3(0.f, 0.f, 0.f);
                const bool on = active && j < K;
                if (on) {
                    float sr[7];
#pragma unroll
                    for (int q = 0; q < 7; q++) sr[q] = s_d2[(7 * j + q) * NGT_LS + a];
                    dof[jj] = ng_cov_delta(sr, s, gof[jj], gxyz[jj], gsc[jj], grot[jj], d, ds, da);   // stored behind the stage's last load (one counter orders both)
                }
                if (j < K) {
#pragma unroll
                    for (int q = 0; q < 7; q++) s_d2[(7 * j + q) * NGT_LS + a] = d[q];
                }
            }
            if (hh == 0) {
#pragma unroll
                for (int q = 7 * K; q < D2R; q++) s_d2[q * NGT_LS + a] = 0.f;
            }
            if (active) {
#pragma unroll
                for (int jj = 0; jj < JH; jj++) {
                    const int j = hh * JH + jj;
                    if (j < K) put3(d_offset, (size_t)i * K + j, dof[jj].x, dof[jj].y, dof[jj].z);
                }
            }
            // the halves' shares of the per-anchor sums meet; d_scaling is complete here, d_anchor waits for the view's share
#pragma unroll
            for (int q = 0; q < 6; q++) ds[q] += __shfl_xor(ds[q], 32);
#pragma unroll
            for (int q = 0; q < 3; q++) da[q] += __shfl_xor(da[q], 32);
            if (active && hh == 0) {
                *reinterpret_cast<row4*>(d_scaling + 6 * (size_t)i) = row4{ds[0], ds[1], ds[2], ds[3]};
                *reinterpret_cast<row2*>(d_scaling + 6 * (size_t)i + 4) = row2{ds[4], ds[5]};
            }
        }
        __builtin_amdgcn_wave_barrier();
        NGT_TICK(3);
        db2 += ngt_bias_sums<7 * K>(s_d2, lane, C_COV);
        NGT_TICK(4);
        ngt_backprop<NG_COV, 7 * K, C_COV, D2R>(sW1, sW2, s_x, s_t, s_d2, lane, dx, g1[NG_COV], g1n[NG_COV >> 1], g2c);
        }
        NGT_TICK(5);
        if constexpr (PASS != 1) {
        // --- opacity (tanh), colour and ray-drop (sigmoid) MLPs
        float ggo[(K + 1) / 2], ggc[(K + 1) / 2], ggr[(K + 1) / 2];
        if constexpr (PASS == 2) {                                     // (as measured: all three heads' rows in front of the first, the first form)
            ngt_small_fetch_cond<K, 0>(active, cidx, hh, slj, g_opacity, g_color, g_no, ggo);
            ngt_small_fetch_cond<K, 1>(active, cidx, hh, slj, g_opacity, g_color, g_no, ggc);
            ngt_small_fetch_cond<K, 2>(active, cidx, hh, slj, g_opacity, g_color, g_no, ggr);
        }
        if constexpr (PASS != 2) ngt_small_fetch<K, 0>(active, cidx, hh, slj, g_opacity, g_color, g_no, ggo);
        ngt_recompute<NG_OPA, K, C_OPA>(sW1, sb1, sW2, sb2, s_x, s_t, s_d2, lane);
        ngt_small_deltas<K, 0>(active, a, hh, ggo, s_d2);
        __builtin_amdgcn_wave_barrier();
        db2 += ngt_bias_sums<K>(s_d2, lane, C_OPA);
        ngt_backprop<NG_OPA, K, C_OPA, D2R>(sW1, sW2, s_x, s_t, s_d2, lane, dx, g1[NG_OPA], g1n[NG_OPA >> 1], g2o);
        if constexpr (PASS != 2) ngt_small_fetch<K, 1>(active, cidx, hh, slj, g_opacity, g_color, g_no, ggc);
        ngt_recompute<NG_COL, K, C_COL>(sW1, sb1, sW2, sb2, s_x, s_t, s_d2, lane);
        ngt_small_deltas<K, 1>(active, a, hh, ggc, s_d2);
        __builtin_amdgcn_wave_barrier();
        db2 += ngt_bias_sums<K>(s_d2, lane, C_COL);
        ngt_backprop<NG_COL, K, C_COL, D2R>(sW1, sW2, s_x, s_t, s_d2, lane, dx, g1[NG_COL], g1n[NG_COL >> 1], g2l);
        if constexpr (PASS != 2) ngt_small_fetch<K, 2>(active, cidx, hh, slj, g_opacity, g_color, g_no, ggr);
        ngt_recompute<NG_RD, K, C_RD>(sW1, sb1, sW2, sb2, s_x, s_t, s_d2, lane);
        ngt_small_deltas<K, 2>(active, a, hh, ggr, s_d2);
        __builtin_amdgcn_wave_barrier();
        db2 += ngt_bias_sums<K>(s_d2, lane, C_RD);
        ngt_backprop<NG_RD, K, C_RD, D2R>(sW1, sW2, s_x, s_t, s_d2, lane, dx, g1[NG_RD], g1n[NG_RD >> 1], g2r);
        }
        NGT_TICK(6);
        // --- input gradients: the feature part leaves in accumulator layout (16 lanes = 64 bytes of an anchor's row); the view /
        //     distance part goes through LDS back to its anchor's lane
        //     (the feature rows of s_x are dead: the tile's dX passes through them, transposed, and leaves as whole 16-byte pieces of rows,
        //     four store instructions per lane instead of sixteen 4-byte ones)
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int aa = 16 * r + 4 * g4 + e;
                s_x[c16 * NGT_LS + aa] = dx[r][0][e]; s_x[(16 + c16) * NGT_LS + aa] = dx[r][1][e];
                if (c16 < 4) s_t[c16 * NGT_LS + aa] = dx[r][2][e];
            }
        __builtin_amdgcn_wave_barrier();
        {
            float4* o4 = reinterpret_cast<float4*>(d_feat) + (size_t)tile * (32 * NG_FEAT / 4);
#pragma unroll
            for (int it = 0; it < 4; it++) {
                const int idx = it * 64 + lane;
                const int aa = idx >> 3, qb = (idx & 7) * 4;
                const float4 v = make_float4(s_x[(qb + 0) * NGT_LS + aa], s_x[(qb + 1) * NGT_LS + aa], s_x[(qb + 2) * NGT_LS + aa], s_x[(qb + 3) * NGT_LS + aa]);
#ifndef LG_NG_T16_NOSTORE
                if (tile * 32 + aa < N && s_act[aa]) {
                    float4 w = v;
                    if (PASS == 1) { const float4 u = pf[it]; w = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w); }
                    o4[idx] = w;
                }
#endif
            }
        }
        if (active && hh == 0) {
            const float4 vd = make_float4(s_x[32 * NGT_LS + a], s_x[33 * NGT_LS + a], s_x[34 * NGT_LS + a], s_x[35 * NGT_LS + a]);   // the tile's own inputs
            ng_view_backward(s_t[0 * NGT_LS + a], s_t[1 * NGT_LS + a], s_t[2 * NGT_LS + a], s_t[3 * NGT_LS + a], vd, da);
            if (PASS == 1) { da[0] += pa.x; da[1] += pa.y; da[2] += pa.z; }
            put3(d_anchor, (size_t)i, da[0], da[1], da[2]);
        }
        __builtin_amdgcn_wave_barrier();
        NGT_TICK(7);
#ifdef LG_NG_T16_DIAG
        tiles_done++;
#endif
    }
#ifdef LG_NG_T16_DIAG
    if (lane == 0 && (blockIdx.x == 3 || blockIdx.x == 200) && (wave == 0 || wave == 5))
        printf("t16 block %d wave %d tiles %d cycles: top %llu staging %llu cov-recompute %llu cov-per-anchor %llu cov-bias-sums %llu cov-backprop %llu three-heads %llu epilogue %llu\n",
               (int)blockIdx.x, wave, tiles_done, tk[0], tk[1], tk[2], tk[3], tk[4], tk[5], tk[6], tk[7]);
#endif
    // ---- the eight waves' sums meet in LDS in wave order; one partial row per workgroup, in k_ng_backward_mfma's layout: tiles
    //      [t or o][q or t] as 32 x 32 blocks (G1 of the four MLPs, their narrow columns, G2 of opacity / covariance / colour /
    //      ray-drop), then the output-layer bias sums
    float* const s_part = s_all + NGT_WEIGHT_FLOATS(K);
    __syncthreads();
    for (int q = tid; q < PER; q += 64 * NGT_WAVES) s_part[q] = 0.f;
    __syncthreads();
    for (int w = 0; w < NGT_WAVES; w++) {
        if (wave == w) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int row = 4 * g4 + e;
#pragma unroll
                for (int mm = 0; mm < 4; mm++) {                       // (a launch adds the tiles of the MLPs it ran; the others stay zero)
                    if ((PASS == 1 && mm != NG_COV) || (PASS == 2 && mm == NG_COV)) continue;
#pragma unroll
                    for (int tr = 0; tr < 2; tr++) {
                        s_part[mm * 1024 + (16 * tr + row) * 32 + c16] += g1[mm][tr][0][e];
                        s_part[mm * 1024 + (16 * tr + row) * 32 + 16 + c16] += g1[mm][tr][1][e];
                    }
                }
#pragma unroll
                for (int p = 0; p < 2; p++) {
                    if (PASS == 1 && p != (NG_COV >> 1)) continue;
#pragma unroll
                    for (int tr = 0; tr < 2; tr++) s_part[4 * 1024 + (16 * tr + row) * 32 + 16 * p + c16] += g1n[p][tr][e];
                }
#pragma unroll
                for (int tc = 0; tc < 2; tc++) {
                    if (PASS != 1) s_part[5 * 1024 + row * 32 + 16 * tc + c16] += g2o[0][tc][e];
                    if (PASS != 2) {
#pragma unroll
                        for (int q = 0; q < ORC; q++) s_part[6 * 1024 + (16 * q + row) * 32 + 16 * tc + c16] += g2c[q][tc][e];
                    }
                    if (PASS != 1) {
                        s_part[(6 + NC) * 1024 + row * 32 + 16 * tc + c16] += g2l[0][tc][e];
                        s_part[(7 + NC) * 1024 + row * 32 + 16 * tc + c16] += g2r[0][tc][e];
                    }
                }
            }
            s_part[(8 + NC) * 1024 + lane] += db2;
        }
        __syncthreads();
    }
    float* out = partial + ((size_t)blockIdx.x + (PASS == 1 ? gridDim.x : 0)) * PER;
    for (int q = tid; q < PER; q += 64 * NGT_WAVES) out[q] = s_part[q];
}


// ---- the forward on the same tiles ------------------------------------------------------------------------------------------------
// k_ng_opacity_mfma / k_ng_decode_mfma run one wave of 64 anchors per workgroup on 32x32x2 tiles with the weights read through L1 and
// 1.8 waves resident per SIMD (LDS): the matrix pipe is busy 37 % of the time, the waves wait for the rest (profiles/r05_j_pmc_sq_decode.json).
// Here (k <= 6): persistent workgroups of twelve waves (three per SIMD), the weights in LDS once per workgroup, a wave = 32 anchors per
// tile on 16x16x4 tiles (ngt_recompute: the backward's own recompute; bias first, inputs in ascending order as in the
// 32x32x2 form -- equal to it to the last bit, not always in it: the matrix pipe orders the four products of a step itself), everything a tile reads requested in one round trip at its top, whole rows per store instruction.  The covariance
// head's outputs land on x (dead behind the last hidden layer), the colour / ray-drop outputs behind x: 48 + 32 rows of 33 floats a wave.
#define NGF_WAVES 12
#define NGF_UROWS(K) ((7 * (K) > 36 + 2 * (K)) ? 7 * (K) : 36 + 2 * (K))
#define NGF_WAVE_FLOATS(K) ((NGF_UROWS(K) + 32) * NGT_LS + 32)

template <int K>
__global__ void __launch_bounds__(64 * NGF_WAVES) k_ng_opacity_t16(int N, NgModel m, float3 cam, const float* __restrict__ feat, const float* __restrict__ anchor,
                                                                   const uint32_t* __restrict__ vis_flags, const uint32_t* __restrict__ vis_idx,
                                                                   float* __restrict__ neural_opacity, uint8_t* __restrict__ mask, uint32_t* __restrict__ sel_flags) {
    __shared__ float s_all[NGT_WEIGHT_FLOATS(K) + NGF_WAVES * NGF_WAVE_FLOATS(K)];
    float* const sW1 = s_all;
    float* const sb1 = sW1 + 128 * NGT_WS;
    float* const sW2 = sb1 + 128;
    float* const sb2 = sW2 + NGT_W2ROWS(K) * NGT_LS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* const s_x = s_all + NGT_WEIGHT_FLOATS(K) + wave * NGF_WAVE_FLOATS(K);
    float* const s_y = s_x + 36 * NGT_LS;
    float* const s_t = s_x + NGF_UROWS(K) * NGT_LS;
    uint32_t* const s_act = reinterpret_cast<uint32_t*>(s_t + 32 * NGT_LS);
    ngt_stage_weights<K, 64 * NGF_WAVES, 1>(m, sW1, sb1, sW2, sb2, tid);
    for (int q = lane; q < NGF_WAVE_FLOATS(K); q += 64) s_x[q] = 0.f;
    __syncthreads();
    constexpr int JH = (K + 1) / 2;
    const int a = lane & 31, hh = lane >> 5;
    const int ntiles = (N + 31) / 32;
    // What a tile reads is requested ONE TILE AHEAD (21 registers this launch has to spare): the round trip runs behind the previous
    // tile's products instead of in front of this one's
    uint32_t pvis = 0u, pcidx = 0u;
    float3 pan = make_float3(0.f, 0.f, 0.f);
    float4 pnf[4];
    auto request = [&](int t) {
        const size_t tt = t < ntiles ? (size_t)t : (size_t)ntiles - 1;  // (past the end: the last tile's words again, never used)
        const size_t i = tt * 32 + a;
        const size_t ic = i < (size_t)N ? i : (size_t)N - 1;            // (unconditional loads from a row every lane may read: see ngt_row)
        pvis = vis_flags[ic]; pcidx = vis_idx[ic]; pan = get3(anchor, ic);
        if (i >= (size_t)N) pvis = 0u;
        const float4* f4 = reinterpret_cast<const float4*>(feat);
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const int idx = it * 64 + lane;
            const size_t ga = tt * 32 + (idx >> 3);
            pnf[it] = f4[(ga < (size_t)N ? ga : (size_t)N - 1) * (NG_FEAT / 4) + (idx & 7)];
        }
    };
    const int tstep = gridDim.x * NGF_WAVES;
    if (blockIdx.x * NGF_WAVES + wave < ntiles) request(blockIdx.x * NGF_WAVES + wave);
    for (int tile = blockIdx.x * NGF_WAVES + wave; tile < ntiles; tile += tstep) {
        const int i = tile * 32 + a;
        const uint32_t vis = pvis, cidx = pcidx;
        const float3 an = pan;
        float4 nf[4];
#pragma unroll
        for (int it = 0; it < 4; it++) nf[it] = pnf[it];
        request(tile + tstep);
        const bool active = vis != 0u;
        if (i < N && !active) {                                        // an anchor off the screen selects nothing
#pragma unroll
            for (int jj = 0; jj < JH; jj++) if (hh * JH + jj < K) sel_flags[(size_t)i * K + hh * JH + jj] = 0u;
        }
        if (__ballot(active) == 0ull) continue;
        __builtin_amdgcn_wave_barrier();
        if (hh == 0) s_act[a] = active ? 1u : 0u;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const int idx = it * 64 + lane;
            const int aa = idx >> 3, qb = (idx & 7) * 4;
            float4 v = nf[it];
            if (!s_act[aa]) v = make_float4(0.f, 0.f, 0.f, 0.f);
            s_x[(qb + 0) * NGT_LS + aa] = v.x; s_x[(qb + 1) * NGT_LS + aa] = v.y; s_x[(qb + 2) * NGT_LS + aa] = v.z; s_x[(qb + 3) * NGT_LS + aa] = v.w;
        }
        if (hh == 0) {
            float4 vd = make_float4(0.f, 0.f, 0.f, 0.f);
            if (active) vd = ng_view(an, cam);
            s_x[32 * NGT_LS + a] = vd.x; s_x[33 * NGT_LS + a] = vd.y; s_x[34 * NGT_LS + a] = vd.z; s_x[35 * NGT_LS + a] = vd.w;
        }
        __builtin_amdgcn_wave_barrier();
        ngt_recompute<NG_OPA, K, ng_col0(NG_OPA, K)>(sW1, sb1, sW2, sb2, s_x, s_t, s_y, lane);
        if (active) {
            float o[JH];
            uint32_t keep[JH];
#pragma unroll
            for (int jj = 0; jj < JH; jj++) {
                const int j = hh * JH + jj < K ? hh * JH + jj : K - 1;
                const NgOpacity r = ng_opacity_out(s_y[j * NGT_LS + a]);
                o[jj] = r.o; keep[jj] = r.keep ? 1u : 0u;
            }
            const size_t w0 = (size_t)cidx * K + hh * JH, f0 = (size_t)i * K + hh * JH;
            if (K == 6) {                                              // (the lane's three offsets are neighbours: one store per array)
                *reinterpret_cast<row3*>(neural_opacity + w0) = row3{o[0], o[1], o[JH - 1]};
                *reinterpret_cast<ngt_u3*>(sel_flags + f0) = ngt_u3{keep[0], keep[1], keep[JH - 1]};
            } else if (K == 4) {
                *reinterpret_cast<row2*>(neural_opacity + w0) = row2{o[0], o[1]};
                *reinterpret_cast<ngt_u2*>(sel_flags + f0) = ngt_u2{keep[0], keep[1]};
            }
#pragma unroll
            for (int jj = 0; jj < JH; jj++) {
                const int j = hh * JH + jj;
                if (j < K) {
                    mask[w0 + jj] = (uint8_t)keep[jj];
                    if (K != 6 && K != 4) { neural_opacity[w0 + jj] = o[jj]; sel_flags[f0 + jj] = keep[jj]; }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

template <int K>
__global__ void __launch_bounds__(64 * NGF_WAVES) k_ng_decode_t16(int N, NgModel m, float3 cam, const float* __restrict__ feat, const float* __restrict__ anchor,
                                                                  const float* __restrict__ offset, const float* __restrict__ scaling,
                                                                  const uint32_t* __restrict__ vis_flags, const uint32_t* __restrict__ vis_idx,
                                                                  const uint32_t* __restrict__ sel_flags, const uint32_t* __restrict__ slot,
                                                                  const float* __restrict__ neural_opacity, float* __restrict__ o_xyz, float* __restrict__ o_color,
                                                                  float* __restrict__ o_opacity, float* __restrict__ o_scaling, float* __restrict__ o_rot) {
    __shared__ float s_all[NGT_WEIGHT_FLOATS(K) + NGF_WAVES * NGF_WAVE_FLOATS(K)];
    float* const sW1 = s_all;
    float* const sb1 = sW1 + 128 * NGT_WS;
    float* const sW2 = sb1 + 128;
    float* const sb2 = sW2 + NGT_W2ROWS(K) * NGT_LS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* const s_x = s_all + NGT_WEIGHT_FLOATS(K) + wave * NGF_WAVE_FLOATS(K);
    float* const s_yc = s_x + 36 * NGT_LS;                             // colour outputs (k rows), ray-drop behind them
    float* const s_yr = s_yc + K * NGT_LS;
    float* const s_t = s_x + NGF_UROWS(K) * NGT_LS;
    uint32_t* const s_act = reinterpret_cast<uint32_t*>(s_t + 32 * NGT_LS);
    ngt_stage_weights<K, 64 * NGF_WAVES, 14>(m, sW1, sb1, sW2, sb2, tid);
    for (int q = lane; q < NGF_WAVE_FLOATS(K); q += 64) s_x[q] = 0.f;
    __syncthreads();
    constexpr int JH = (K + 1) / 2;
    const int a = lane & 31, hh = lane >> 5;
    const int ntiles = (N + 31) / 32;
    for (int tile = blockIdx.x * NGF_WAVES + wave; tile < ntiles; tile += gridDim.x * NGF_WAVES) {
        const int i = tile * 32 + a;
        // everything the tile reads, in one round trip (the opacities of the selected pairs wait for the compact index: a second one, behind
        // which the MLPs run)
        uint32_t vis = 0u, cidx = 0u, nsel[JH], nslot[JH];
        float3 an = make_float3(0.f, 0.f, 0.f), of[JH];
        float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float4 nf[4];
#pragma unroll
        for (int jj = 0; jj < JH; jj++) { nsel[jj] = 0u; nslot[jj] = 0u; of[jj] = make_float3(0.f, 0.f, 0.f); }
        {
            const size_t ic = i < N ? i : N - 1;                       // (unconditional loads from a row every lane may read: see ngt_row)
            vis = vis_flags[ic]; cidx = vis_idx[ic]; an = get3(anchor, ic);
            if (i >= N) vis = 0u;
            const row4 sa = *reinterpret_cast<const row4*>(scaling + 6 * ic);
            const row2 sb = *reinterpret_cast<const row2*>(scaling + 6 * ic + 4);
            s[0] = sa.x; s[1] = sa.y; s[2] = sa.z; s[3] = sa.w; s[4] = sb.x; s[5] = sb.y;
#pragma unroll
            for (int jj = 0; jj < JH; jj++) {
                const int j = hh * JH + jj, jc = j < K ? j : K - 1;
                nsel[jj] = sel_flags[ic * K + jc]; nslot[jj] = slot[ic * K + jc]; of[jj] = get3(offset, ic * K + jc);
                if (j >= K) nsel[jj] = 0u;
            }
            const float4* f4 = reinterpret_cast<const float4*>(feat);
#pragma unroll
            for (int it = 0; it < 4; it++) {
                const int idx = it * 64 + lane;
                const size_t ga = (size_t)tile * 32 + (idx >> 3);
                nf[it] = f4[(ga < (size_t)N ? ga : (size_t)N - 1) * (NG_FEAT / 4) + (idx & 7)];
            }
        }
        bool own = false;
#pragma unroll
        for (int jj = 0; jj < JH; jj++) own = own || (vis != 0u && nsel[jj] != 0u);
        const int other = __shfl_xor((int)own, 32);                   // the two halves of an anchor agree (no short circuit around the exchange)
        const bool active = own || other != 0;
        if (__ballot(active) == 0ull) continue;
        float nop[JH];
#pragma unroll
        for (int jj = 0; jj < JH; jj++) {                             // (a visible anchor's compact index is a row of neural_opacity's)
            const int j = hh * JH + jj, jc = j < K ? j : K - 1;
            nop[jj] = neural_opacity[(size_t)(vis != 0u ? cidx : 0u) * K + jc];     // :71
        }
        __builtin_amdgcn_wave_barrier();
        if (hh == 0) s_act[a] = active ? 1u : 0u;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const int idx = it * 64 + lane;
            const int aa = idx >> 3, qb = (idx & 7) * 4;
            float4 v = nf[it];
            if (!s_act[aa]) v = make_float4(0.f, 0.f, 0.f, 0.f);
            s_x[(qb + 0) * NGT_LS + aa] = v.x; s_x[(qb + 1) * NGT_LS + aa] = v.y; s_x[(qb + 2) * NGT_LS + aa] = v.z; s_x[(qb + 3) * NGT_LS + aa] = v.w;
        }
        if (hh == 0) {
            float4 vd = make_float4(0.f, 0.f, 0.f, 0.f);
            if (active) vd = ng_view(an, cam);
            s_x[32 * NGT_LS + a] = vd.x; s_x[33 * NGT_LS + a] = vd.y; s_x[34 * NGT_LS + a] = vd.z; s_x[35 * NGT_LS + a] = vd.w;
        }
        __builtin_amdgcn_wave_barrier();
        ngt_recompute<NG_COL, K, ng_col0(NG_COL, K)>(sW1, sb1, sW2, sb2, s_x, s_t, s_yc, lane);
        ngt_recompute<NG_RD, K, ng_col0(NG_RD, K)>(sW1, sb1, sW2, sb2, s_x, s_t, s_yr, lane);
        float colv[JH], rdv[JH];                                       // (the covariance outputs overwrite these rows too)
#pragma unroll
        for (int jj = 0; jj < JH; jj++) {
            const int j = hh * JH + jj < K ? hh * JH + jj : K - 1;
            colv[jj] = s_yc[j * NGT_LS + a]; rdv[jj] = s_yr[j * NGT_LS + a];
        }
        __builtin_amdgcn_wave_barrier();
        ngt_recompute<NG_COV, 7 * K, ng_col0(NG_COV, K)>(sW1, sb1, sW2, sb2, s_x, s_t, s_x, lane);     // its outputs land on x (dead behind the hidden layer)
#pragma unroll
        for (int jj = 0; jj < JH; jj++) {
            const int j = hh * JH + jj;
            if (j < K && vis != 0u && nsel[jj] != 0u) {
                const size_t r = nslot[jj];
                float sr[7];
#pragma unroll
                for (int q = 0; q < 7; q++) sr[q] = s_x[(7 * j + q) * NGT_LS + a];
                const NgRow v = ng_decode_row(an, of[jj], s, colv[jj], rdv[jj], sr);
                put3(o_xyz, r, v.xyz.x, v.xyz.y, v.xyz.z);
                put2(o_color, r, v.color.x, v.color.y);
                o_opacity[r] = nop[jj];
                put3(o_scaling, r, v.scaling.x, v.scaling.y, v.scaling.z);
                put4(o_rot, r, v.rot.x, v.rot.y, v.rot.z, v.rot.w);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}
