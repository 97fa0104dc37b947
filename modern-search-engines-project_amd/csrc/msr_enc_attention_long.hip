// Encoder attention for long sequences (document chunks: 514 tokens, up to ModernBERT's 8192), include/msretr_encoder.h
// msr_enc_attention_long.  Same arguments and arithmetic contract as msr_enc_attention (csrc/msr_encoder.hip), whose
// kernels keep one sequence's whole K / V in LDS and so stop at 128 tokens.
//
// Flash-style: one workgroup per (sequence, head, 64-row query tile), 4 waves of 16 query rows.  K (rotary embedding
// applied) and V are streamed through LDS in tiles of 64 keys; each wave keeps its 16 rows' q in registers and a running
// maximum / denominator per row (online softmax, f32).  A local layer (window > 0) visits only the key tiles that meet
// [q0 - window, q0 + 63 + window]: 3 tiles for window 64, so its cost is linear in the length.
//
// Both products run on v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation: a k-ordered fmaf chain).  Operand
// maps (lane l, g = l >> 4, c = l & 15; A[i = c][k = g], B[k = g][j = c], D[row 4 g + r][col c]):
//   S^T = K . Q^T   per 16-key block kb: A = K[kb*16 + c][feature], B = q[query c][feature], feature 16 g + s in step s
//                   -> lane holds the scores of query c against keys kb*16 + 4 g + r (r = 0..3).
//   O^T = V^T . P^T per 16-feature block nb, step (kb, r): A = V[kb*16 + 4 g + r][nb*16 + c], B = the lane's own weight of
//                   key kb*16 + 4 g + r -> lane holds O[query c][nb*16 + 4 g + r].
// So a lane's scores, weights, running statistics and outputs all belong to query c: no lane exchange except the row
// maximum and the final denominator (xor 16, xor 32).
#include <math.h>

#include "../../include/msretr.h"
#include "../../include/msretr_encoder.h"
#include "msr_common.h"
#include "msr_internal.h"

namespace {

constexpr int HEAD_DIM = 64;
constexpr int QT = 64;                  // query rows per workgroup (4 waves x 16)
constexpr int KT = 64;                  // keys per LDS tile
constexpr int LD = HEAD_DIM + 4;        // LDS row pitch (floats): a 4-key step of the V reads moves 16 banks
constexpr int LONG_MAX_SEQ = 8192;      // ModernBERT max_position_embeddings

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void enc_attention_long_kernel(const float* __restrict__ qkv,
                                                                 const int32_t* __restrict__ seq_off, int n_heads, int n_qt,
                                                                 const float* __restrict__ inv_freq, int window, int bound,
                                                                 float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float Ks[KT][LD];
    __shared__ __attribute__((aligned(16))) float Vs[KT][LD];
    const int64_t blk = blockIdx.x;
    const int qt = (int)(blk % n_qt);
    const int64_t bh = blk / n_qt;
    const int h = (int)(bh % n_heads);
    const int b = (int)(bh / n_heads);
    const int t0 = seq_off[b], S = seq_off[b + 1] - t0;
    const int ld_out = n_heads * HEAD_DIM;
    const int64_t stride = 3 * (int64_t)ld_out;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (S > bound) {                                             // longer than the caller's bound: NaN rows, read nothing
        if (qt == 0) {                                           // (S is block-uniform; tile 0 writes the whole sequence)
            float* o = out + (int64_t)t0 * ld_out + h * HEAD_DIM;
            for (int64_t i = tid; i < (int64_t)S * HEAD_DIM; i += 256)
                o[(i / HEAD_DIM) * ld_out + (i % HEAD_DIM)] = __builtin_nanf("");
        }
        return;
    }
    const int q0 = qt * QT;
    if (q0 >= S) return;
    const float* base = qkv + (int64_t)t0 * stride + h * HEAD_DIM;     // q of token 0 of the sequence, head h
    const int k_off = ld_out, v_off = 2 * ld_out;

    // ---- q of this lane's query row (c), features 16 g .. 16 g + 15, rotated; zero past the end of the sequence.
    // rotate-half: x'_j = x_j cos_j - x_{j+32} sin_j (j < 32), x'_j = x_j cos_{j-32} + x_{j-32} sin_{j-32} (j >= 32),
    // angle_j = position * inv_freq[j] -- the operations of msr_enc_attention, in the same order.
    const int c = lane & 15, g = lane >> 4;
    const int t = q0 + wave * 16 + c;                            // this lane's query position
    float qf[16];
    if (t < S) {
        const float* qp = base + (int64_t)t * stride;
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const f32x4 x = *(const f32x4*)(qp + 16 * g + 4 * s4);
            const f32x4 y = *(const f32x4*)(qp + ((16 * g) ^ 32) + 4 * s4);      // rotation partners
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = (16 * g + 4 * s4 + e) & 31;
                const float ang = (float)t * inv_freq[j];
                const float cs = cosf(ang), sn = sinf(ang);
                qf[4 * s4 + e] = g < 2 ? x[e] * cs - y[e] * sn : x[e] * cs + y[e] * sn;
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < 16; ++s) qf[s] = 0.f;
    }

    // ---- key tiles to visit
    int k_lo = 0, k_hi = S;
    if (window > 0) {
        const int last = min(S - 1, q0 + QT - 1);
        k_lo = max(0, q0 - window);
        k_hi = min(S, last + window + 1);
    }
    const int kt_lo = k_lo / KT, kt_hi = (k_hi + KT - 1) / KT;

    // tile loader: thread -> key kk = tid >> 2, features [8 p, 8 p + 8) and their partners [32 + 8 p, 32 + 8 p + 8)
    const int kk = tid >> 2, p = tid & 3;
    f32x4 kr[4], vr[4];
    auto load_raw = [&](int kt) {
        const int key = kt * KT + kk;
        if (key < S) {
            const float* kp = base + (int64_t)key * stride + k_off;
            const float* vp = base + (int64_t)key * stride + v_off;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                kr[i] = *(const f32x4*)(kp + 8 * p + 4 * i);
                kr[2 + i] = *(const f32x4*)(kp + 32 + 8 * p + 4 * i);
                vr[i] = *(const f32x4*)(vp + 8 * p + 4 * i);
                vr[2 + i] = *(const f32x4*)(vp + 32 + 8 * p + 4 * i);
            }
        } else {                                                 // past the end: zeros (weight 0 x finite v)
#pragma unroll
            for (int i = 0; i < 4; ++i) kr[i] = vr[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_tile = [&](int kt) {
        const float pos = (float)(kt * KT + kk);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            f32x4 lo, hi;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ang = pos * inv_freq[8 * p + 4 * i + e];
                const float cs = cosf(ang), sn = sinf(ang);
                const float k1 = kr[i][e], k2 = kr[2 + i][e];
                lo[e] = k1 * cs - k2 * sn;
                hi[e] = k2 * cs + k1 * sn;
            }
            *(f32x4*)&Ks[kk][8 * p + 4 * i] = lo;
            *(f32x4*)&Ks[kk][32 + 8 * p + 4 * i] = hi;
            *(f32x4*)&Vs[kk][8 * p + 4 * i] = vr[i];
            *(f32x4*)&Vs[kk][32 + 8 * p + 4 * i] = vr[2 + i];
        }
    };

    f32x4 o[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) o[nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float mx = -INFINITY, den = 0.f;                             // den: this lane's share (keys 4 g + r of every block)

    load_raw(kt_lo);
    for (int kt = kt_lo; kt < kt_hi; ++kt) {
        __syncthreads();                                         // every wave is done with the previous tile
        store_tile(kt);
        __syncthreads();
        if (kt + 1 < kt_hi) load_raw(kt + 1);                    // next tile's loads in flight during this one's products

        // S^T = K . Q^T, four blocks of 16 keys
        f32x4 sc[4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            sc[kb] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const float* kp = &Ks[kb * 16 + c][16 * g];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const f32x4 kv = *(const f32x4*)(kp + 4 * s4);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    sc[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[e], qf[4 * s4 + e], sc[kb], 0, 0, 0);
            }
        }
        // mask, scale, tile maximum of row c
        float m_tile = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kt * KT + kb * 16 + 4 * g + r;
                const int dist = key > t ? key - t : t - key;
                const bool keep = key < S && !(window > 0 && dist > window);
                const float v = keep ? sc[kb][r] * 0.125f : -INFINITY;       // head_dim ** -0.5
                sc[kb][r] = v;
                m_tile = fmaxf(m_tile, v);
            }
        m_tile = fmaxf(m_tile, __shfl_xor(m_tile, 16));
        m_tile = fmaxf(m_tile, __shfl_xor(m_tile, 32));
        const float m_new = fmaxf(mx, m_tile);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;    // no key kept yet: weights 0, nothing to rescale
        const float scale = expf(mx - m_use);                    // first kept key: exp(-inf) = 0
        mx = m_new;
        float psum = 0.f;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = expf(sc[kb][r] - m_use);
                sc[kb][r] = e;
                psum += e;
            }
        den = den * scale + psum;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) o[nb] *= scale;
        // O^T += V^T . P^T
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* vp = &Vs[kb * 16 + 4 * g + r][c];
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
                    o[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[nb * 16], sc[kb][r], o[nb], 0, 0, 0);
            }
    }
    den += __shfl_xor(den, 16);
    den += __shfl_xor(den, 32);
    if (t < S) {
        float* op = out + (int64_t)(t0 + t) * ld_out + h * HEAD_DIM + 4 * g;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = o[nb][e] / den;
            *(f32x4*)(op + nb * 16) = y;
        }
    }
}

}  // namespace

extern "C" int msr_enc_attention_long(const float* qkv, const int32_t* seq_off, int32_t n_seq, int32_t n_heads,
                                      const float* inv_freq, int32_t window, int32_t max_len, float* out, void* stream) {
    if (!qkv || !seq_off || !inv_freq || !out || n_seq < 0 || n_heads < 1 || n_heads > 64 || max_len < 0 ||
        max_len > LONG_MAX_SEQ || ((uintptr_t)qkv & 15) || ((uintptr_t)out & 15))
        return msr_fail_global(MSR_ERR_INVALID, "msr_enc_attention_long: bad argument (max_len=%d; <= %d, 16-byte aligned "
                               "qkv / out)", max_len, LONG_MAX_SEQ);
    if (n_seq == 0) return MSR_OK;
    const int bound = max_len > 0 ? max_len : LONG_MAX_SEQ;
    const int n_qt = (bound + QT - 1) / QT;
    const int64_t blocks = (int64_t)n_seq * n_heads * n_qt;
    if (blocks > 0x7fffffff)
        return msr_fail_global(MSR_ERR_INVALID, "msr_enc_attention_long: %lld workgroups", (long long)blocks);
    enc_attention_long_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(qkv, seq_off, n_heads, n_qt, inv_freq,
                                                                                 window, bound, out);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? MSR_OK : msr_fail_global(MSR_ERR_HIP, "msr_enc_attention_long: %s", hipGetErrorString(err));
}
