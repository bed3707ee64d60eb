// Decode-step kernels of the branch-batched LLaVA language model for gfx950 (MI355X).
//
// They replace what the reference executes, per branch and per token, through HF's eager
// LlamaModel (experiments/llava/model/language_model/llava_llama.py:88-103 -> transformers
// LlamaDecoderLayer [ext]).  Rows of one step = (question, branch) pairs, so the weights are
// streamed from HBM once per step for ALL branches (the reference streams them once per
// branch: vcd_sample.py:109,163,178).  Compiled once per storage type (bf16 / fp16, csrc/vdd_elem.h); accumulation fp32.
//
//   vdd_rmsnorm                    h = residual(+delta | + fp32 slabs); y = h * rsqrt(mean h^2 + eps) * w
//   vdd_rope_kv_write              RoPE(q,k) at per-row positions; k,v -> per-row KV slot
//   vdd_rope_kv_write_paged        ... k,v -> the paged own-KV pool
//   vdd_kv_pages_scatter           contiguous own slots -> pages
//   vdd_silu_mul                   silu(gate) * up
//   vdd_embed, vdd_embed_scatter   token embedding gather
//   vdd_skinny_gemm                Y[M,N] = X[M,K] W[N,K]^T (+R | fp32 split-K slabs), M <= 64: weight streaming (W read once; MFMA
//                                  16x16x32 does the k-reduction): skinny_gemm_kernel, skinny_wide_kernel at 17 - 64 rows and N > 8192
//   vdd_skinny_swiglu              act = silu(X Wg^T) * (X Wu^T): skinny_swiglu_kernel, skinny_wide_kernel at 17 - 64 rows
//   vdd_skinny_gemm_resid_ss       M <= 16: Y = X W^T + R and the sum of squares of Y's rows (skinny_gemm_kernel, SSOUT)
//   vdd_skinny_gemm_normed         M <= 16: Y = rmsnorm(H) W^T from those sums of squares (skinny_normed_kernel)
//   vdd_skinny_swiglu_normed       M <= 16: the same with the SwiGLU epilogue
//   vdd_skinny_gemm_resid_ss_w8, vdd_skinny_gemm_normed_w8, vdd_skinny_swiglu_normed_w8
//                                  the same three on e4m3 weights (vdd_w8.h)
//
// All HBM-bound.  The step's attention is in vdd_decode_attention.hip.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vdd_llm_common.h"
#include "vdd_w8.h"

namespace {
namespace VDD_ELEM_NS {

// a weight fragment of the weight-streaming projections: every byte of W is read by ONE wave, once per launch.  Default cache policy:
// nontemporal weight loads measured SLOWER here (one-question layer chain 90.2 vs 84.8 us)
__device__ __forceinline__ frag8_t ld_w(const uint16_t* p) { return *reinterpret_cast<const frag8_t*>(p); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// the NW wave partials p[0], p[stride], ... of one entry, added in a fixed tree: deterministic
template <int NW>
__device__ __forceinline__ float wave_partial_sum(const float* p, int stride) {
    float s = (p[0] + p[stride]) + (p[2 * stride] + p[3 * stride]);
    if constexpr (NW == 8) s += (p[4 * stride] + p[5 * stride]) + (p[6 * stride] + p[7 * stride]);
    return s;
}
// SwiGLU epilogue from the fp32 sums of the gate and the up column, with the rounding points of the unfused pair:
// gate, up -> element type; silu(gate) -> element type; product -> element type
__device__ __forceinline__ uint16_t swiglu_out(float gs, float us) {
    const float gb = e2f(f2e(gs)), ub = e2f(f2e(us));
    const float sl = e2f(f2e(gb / (1.f + __expf(-gb))));
    return (uint16_t)f2e(sl * ub);
}

// ------------------------------------------------------------------ RMSNorm (+ residual add)
// One 256-thread block per row; the row stays in registers between the two passes.
// HF rounding order: h = bf16(resid + delta); y = bf16( bf16(h * rstd) * w ).
template <int VPT>   // uint4 (8 x bf16) per thread
__global__ void __launch_bounds__(256) rmsnorm_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ delta,
                                                      const float* __restrict__ slabs, int n_slabs, long long slab_stride,
                                                      const uint16_t* __restrict__ w, uint16_t* __restrict__ y,
                                                      uint16_t* __restrict__ resid_out, int d, float eps, int stream) {
    __shared__ float red[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    const size_t off = (size_t)row * d;
    uint4 h[VPT], dl[VPT], wv[VPT];
    float ss = 0.f;
    // every load of the row leaves before anything is consumed (x, the delta, the ln weights: ONE memory round trip), from clamped,
    // never predicated addresses: a load inside `if (e < d)` is waited for inside that branch, which made the VPT chunks of a thread
    // - and the weights behind them - a chain of round trips (13 us for 25 MB at 1,536 rows)
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int e = (i * 256 + tid) * 8, ec = e < d ? e : 0;
        h[i] = stream ? ld_stream(x + off + ec) : *reinterpret_cast<const uint4*>(x + off + ec);
        if (delta != nullptr) dl[i] = stream ? ld_stream(delta + off + ec) : *reinterpret_cast<const uint4*>(delta + off + ec);
        wv[i] = *reinterpret_cast<const uint4*>(w + ec);
    }
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int e = (i * 256 + tid) * 8;
        if (e < d) {
            uint4 a = h[i];
            if (delta != nullptr) {
                const uint4 b = dl[i];
                a.x = pack(lo(a.x) + lo(b.x), hi(a.x) + hi(b.x)); a.y = pack(lo(a.y) + lo(b.y), hi(a.y) + hi(b.y));
                a.z = pack(lo(a.z) + lo(b.z), hi(a.z) + hi(b.z)); a.w = pack(lo(a.w) + lo(b.w), hi(a.w) + hi(b.w));
            }
            if (slabs != nullptr) {      // delta = bf16(sum of the split-K fp32 partial slabs of the producing GEMM)
                float dsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                // the slabs are added in slab order (the bits of round 4), but their loads go out FOUR slabs at a time: one slab per iteration
                // was one memory round trip per slab (S = 8 - 27: most of this launch's time at a few dozen rows)
                int sl = 0;
                for (; sl + 4 <= n_slabs; sl += 4) {
                    float4 q0[4], q1[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        q0[u] = *reinterpret_cast<const float4*>(slabs + (size_t)(sl + u) * slab_stride + off + e);
                        q1[u] = *reinterpret_cast<const float4*>(slabs + (size_t)(sl + u) * slab_stride + off + e + 4);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        dsum[0] += q0[u].x; dsum[1] += q0[u].y; dsum[2] += q0[u].z; dsum[3] += q0[u].w;
                        dsum[4] += q1[u].x; dsum[5] += q1[u].y; dsum[6] += q1[u].z; dsum[7] += q1[u].w;
                    }
                }
                for (; sl < n_slabs; ++sl) {
                    const float4 p0 = *reinterpret_cast<const float4*>(slabs + (size_t)sl * slab_stride + off + e);
                    const float4 p1 = *reinterpret_cast<const float4*>(slabs + (size_t)sl * slab_stride + off + e + 4);
                    dsum[0] += p0.x; dsum[1] += p0.y; dsum[2] += p0.z; dsum[3] += p0.w;
                    dsum[4] += p1.x; dsum[5] += p1.y; dsum[6] += p1.z; dsum[7] += p1.w;
                }
                auto addr = [&](uint32_t hv, float d0, float d1) { return pack(lo(hv) + e2f(f2e(d0)), hi(hv) + e2f(f2e(d1))); };
                a.x = addr(a.x, dsum[0], dsum[1]); a.y = addr(a.y, dsum[2], dsum[3]);
                a.z = addr(a.z, dsum[4], dsum[5]); a.w = addr(a.w, dsum[6], dsum[7]);
            }
            if (resid_out != nullptr) { if (stream) st_stream(resid_out + off + e, a); else *reinterpret_cast<uint4*>(resid_out + off + e) = a; }
            h[i] = a;
            float f;
            f = lo(a.x); ss += f * f; f = hi(a.x); ss += f * f; f = lo(a.y); ss += f * f; f = hi(a.y); ss += f * f;
            f = lo(a.z); ss += f * f; f = hi(a.z); ss += f * f; f = lo(a.w); ss += f * f; f = hi(a.w); ss += f * f;
        }
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    const float rstd = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)d + eps);
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int e = (i * 256 + tid) * 8;
        if (e < d) {
            uint4 a = h[i], g = wv[i], o;
            auto nrm = [&](uint32_t hv, uint32_t gv) {
                float n0 = e2f(f2e(lo(hv) * rstd)), n1 = e2f(f2e(hi(hv) * rstd));
                return pack(n0 * lo(gv), n1 * hi(gv));
            };
            o.x = nrm(a.x, g.x); o.y = nrm(a.y, g.y); o.z = nrm(a.z, g.z); o.w = nrm(a.w, g.w);
            *reinterpret_cast<uint4*>(y + off + e) = o;
        }
    }
}

// ------------------------------------------------------------------ RoPE + KV-cache write
// qkv: [M, (Hq + 2 Hkv) * D] (q | k | v).  One block per row, one 16-lane group per head
// chunk.  rotate_half pairing (HF Llama): (i, i + D/2).  cos/sin table: fp32 [max_pos, D/2].
// K/V go to cache[slot][kv_head][pos][D].
// The row's work, shared by the contiguous and the paged kernel: p = rotary position; (s, cp) = cache slot and index inside it
// (a page and the index inside the page for the paged pool); write_kv = false (block-uniform) leaves the caches alone.
__device__ __forceinline__ void rope_kv_row(const uint16_t* __restrict__ qkv, const float* __restrict__ cs_table,
                                            uint16_t* __restrict__ q_out, uint16_t* __restrict__ k_cache,
                                            uint16_t* __restrict__ v_cache, int Hq, int Hkv, int D, long long slot_stride,
                                            int t_max, int stream, int row, int p, int s, int cp, bool write_kv) {
    const int tid = threadIdx.x;
    const int half = D / 2, h8 = half / 8;                      // a work item = 8 consecutive pairs (i, i + D/2) of one head
    const uint16_t* src = qkv + (size_t)row * (size_t)((Hq + 2 * Hkv) * D);
    const float* cs = cs_table + (size_t)p * half * 2;
    // All loads of a pass leave before the first result is used: work items tid, tid + 256, ... in batches of IT, read from clamped
    // (always valid) indices, consumed under the `valid` predicate.  As `for (i = tid; i < n; i += 256) { load; rotate; store; }` every
    // trip was a memory round trip of its own (two for q / k, two for v: 17 us per launch at 1,536 rows).
    constexpr int IT = 2;                                     // 64 q / k heads x 8 items = 512 = one batch
    const int n_qk = (Hq + Hkv) * h8;
    for (int i0 = tid; i0 < n_qk; i0 += 256 * IT) {
        uint4 a4[IT], b4[IT];
        float4 c[IT][4];
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int i = i0 + 256 * k, ic = i < n_qk ? i : 0;
            const int head = ic / h8, pi = (ic % h8) * 8;
            const uint16_t* hsrc = src + (size_t)head * D;           // q heads then k heads are contiguous in qkv
            a4[k] = stream ? ld_stream(hsrc + pi) : *reinterpret_cast<const uint4*>(hsrc + pi);
            b4[k] = stream ? ld_stream(hsrc + pi + half) : *reinterpret_cast<const uint4*>(hsrc + pi + half);
#pragma unroll
            for (int q = 0; q < 4; ++q) c[k][q] = *reinterpret_cast<const float4*>(cs + pi * 2 + 4 * q);
        }
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int i = i0 + 256 * k;
            if (i < n_qk) {
                const int head = i / h8, pi = (i % h8) * 8;
                const bool is_k = head >= Hq;
                auto rot = [](uint32_t av, uint32_t bv, float cA, float sA, float cB, float sB, uint32_t& r0, uint32_t& r1) {
                    const float a0 = lo(av), a1 = hi(av), b0 = lo(bv), b1 = hi(bv);
                    r0 = pack(a0 * cA - b0 * sA, a1 * cB - b1 * sB);
                    r1 = pack(b0 * cA + a0 * sA, b1 * cB + a1 * sB);
                };
                uint4 r0, r1;
                rot(a4[k].x, b4[k].x, c[k][0].x, c[k][0].y, c[k][0].z, c[k][0].w, r0.x, r1.x);
                rot(a4[k].y, b4[k].y, c[k][1].x, c[k][1].y, c[k][1].z, c[k][1].w, r0.y, r1.y);
                rot(a4[k].z, b4[k].z, c[k][2].x, c[k][2].y, c[k][2].z, c[k][2].w, r0.z, r1.z);
                rot(a4[k].w, b4[k].w, c[k][3].x, c[k][3].y, c[k][3].z, c[k][3].w, r0.w, r1.w);
                uint16_t* dst = is_k ? k_cache + (size_t)s * slot_stride + ((size_t)(head - Hq) * t_max + cp) * D
                                     : q_out + (size_t)row * Hq * D + (size_t)head * D;
                if (is_k && !write_kv) continue;
                if (is_k && stream) { st_stream(dst + pi, r0); st_stream(dst + pi + half, r1); }
                else { *reinterpret_cast<uint4*>(dst + pi) = r0; *reinterpret_cast<uint4*>(dst + pi + half) = r1; }
            }
        }
    }
    if (!write_kv) return;
    const uint16_t* vsrc = src + (size_t)(Hq + Hkv) * D;
    const int n_v = Hkv * D / 8;
    for (int i0 = tid; i0 < n_v; i0 += 256 * IT) {
        uint4 vv[IT];
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int i = i0 + 256 * k, ic = i < n_v ? i : 0;
            vv[k] = stream ? ld_stream(vsrc + (size_t)ic * 8) : *reinterpret_cast<const uint4*>(vsrc + (size_t)ic * 8);
        }
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int i = i0 + 256 * k;
            if (i < n_v) {
                const int head = (i * 8) / D, dd = (i * 8) % D;
                uint16_t* vd = v_cache + (size_t)s * slot_stride + ((size_t)head * t_max + cp) * D + dd;
                if (stream) st_stream(vd, vv[k]); else *reinterpret_cast<uint4*>(vd) = vv[k];
            }
        }
    }
}

__global__ void __launch_bounds__(256) rope_kv_kernel(const uint16_t* __restrict__ qkv, const int* __restrict__ pos,
                                                      const int* __restrict__ cpos, const int* __restrict__ slot,
                                                      const float* __restrict__ cs_table,
                                                      uint16_t* __restrict__ q_out, uint16_t* __restrict__ k_cache,
                                                      uint16_t* __restrict__ v_cache, int Hq, int Hkv, int D,
                                                      long long slot_stride, int t_max, int stream) {
    const int row = blockIdx.x;
    rope_kv_row(qkv, cs_table, q_out, k_cache, v_cache, Hq, Hkv, D, slot_stride, t_max, stream, row, pos[row], slot[row], cpos[row], true);
}

// Paged own-KV pool (PageTable, vdd_llm_common.h): a page is a KV_PAGE-token cache slot, so the row's work is rope_kv_row with
// (slot, index) = (page, i % KV_PAGE).  No page (entry < 0), or anything out of range: q is still rotated, K / V are not stored.
__global__ void __launch_bounds__(256) rope_kv_paged_kernel(const uint16_t* __restrict__ qkv, const int* __restrict__ pos,
                                                            const int* __restrict__ cpos, const int* __restrict__ slot,
                                                            const float* __restrict__ cs_table, uint16_t* __restrict__ q_out,
                                                            uint16_t* __restrict__ k_pages, uint16_t* __restrict__ v_pages,
                                                            PageTable pt, int Hq, int Hkv, int D, int stream) {
    const int row = blockIdx.x, cp = cpos[row];
    const int pg = page_of(pt, slot[row], cp);
    rope_kv_row(qkv, cs_table, q_out, k_pages, v_pages, Hq, Hkv, D, (long long)Hkv * KV_PAGE * D, KV_PAGE, stream, row, pos[row],
                pg < 0 ? 0 : pg, cp & (KV_PAGE - 1), pg >= 0);
}

// Contiguous own slots -> pages (the admission prefill writes a question's suffix K / V into a short contiguous staging slot):
// block (i, r) copies own token i < n_tok[r] of slot slots[r], all KV heads, K and V, 16 bytes per lane.
__global__ void __launch_bounds__(256) kv_pages_scatter_kernel(const uint16_t* __restrict__ k_own, const uint16_t* __restrict__ v_own,
                                                               uint16_t* __restrict__ k_pages, uint16_t* __restrict__ v_pages,
                                                               PageTable pt, const int* __restrict__ slots,
                                                               const int* __restrict__ n_tok, int Hkv, int D, long long slot_stride,
                                                               int t_max, int n_own) {
    const int i = blockIdx.x, r = blockIdx.y, s = slots[r];
    if (i >= n_tok[r] || i >= t_max || s < 0 || s >= n_own) return;
    const int pg = page_of(pt, s, i);
    if (pg < 0) return;
    const int d8 = D / 8;
    for (int e = threadIdx.x; e < Hkv * d8; e += 256) {
        const int head = e / d8, dd = (e % d8) * 8;
        const size_t src = (size_t)s * slot_stride + ((size_t)head * t_max + i) * D + dd;
        const size_t dst = ((size_t)pg * Hkv + head) * KV_PAGE * D + (size_t)(i & (KV_PAGE - 1)) * D + dd;
        *reinterpret_cast<uint4*>(k_pages + dst) = *reinterpret_cast<const uint4*>(k_own + src);
        *reinterpret_cast<uint4*>(v_pages + dst) = *reinterpret_cast<const uint4*>(v_own + src);
    }
}

// ------------------------------------------------------------------ SiLU(gate) * up
__global__ void __launch_bounds__(256) silu_mul_kernel(const uint16_t* __restrict__ gu, uint16_t* __restrict__ out,
                                                       long long M, int F) {
    // grid: (ceil(F / 8 / 256), M): a thread owns 8 consecutive features of one row
    const int f = (blockIdx.x * 256 + threadIdx.x) * 8;
    if (f >= F) return;
    const size_t m = blockIdx.y;
    const uint4 g = *reinterpret_cast<const uint4*>(gu + m * 2 * F + f);
    const uint4 u = *reinterpret_cast<const uint4*>(gu + m * 2 * F + F + f);
    auto act = [](uint32_t gv, uint32_t uv) {
        const float g0 = lo(gv), g1 = hi(gv);
        const float s0 = e2f(f2e(g0 / (1.f + __expf(-g0)))), s1 = e2f(f2e(g1 / (1.f + __expf(-g1))));
        return pack(s0 * lo(uv), s1 * hi(uv));
    };
    uint4 o; o.x = act(g.x, u.x); o.y = act(g.y, u.y); o.z = act(g.z, u.z); o.w = act(g.w, u.w);
    *reinterpret_cast<uint4*>(out + m * F + f) = o;
}

// ------------------------------------------------------------------ embedding gather
// ids outside [0, vocab) read row 0 instead of wild memory: a row whose distribution had no finite score gets token -1
// from the sampling kernel (its status is what the host raises on), and the captured decode step embeds it before any check
__global__ void __launch_bounds__(256) embed_kernel(const long long* __restrict__ ids, const uint16_t* __restrict__ table,
                                                    uint16_t* __restrict__ out, int d, int vocab) {
    const int row = blockIdx.x;
    long long id = ids[row];
    if (id < 0 || id >= vocab) id = 0;
    for (int e = threadIdx.x * 8; e < d; e += 256 * 8)
        *reinterpret_cast<uint4*>(out + (size_t)row * d + e) = *reinterpret_cast<const uint4*>(table + (size_t)id * d + e);
}

__global__ void __launch_bounds__(256) embed_scatter_kernel(const int* __restrict__ ids, const int* __restrict__ rows,
                                                            const uint16_t* __restrict__ table, uint16_t* __restrict__ out, int d, int vocab) {
    long long id = ids[blockIdx.x];
    if (id < 0 || id >= vocab) id = 0;
    const size_t row = (size_t)rows[blockIdx.x];
    for (int e = threadIdx.x * 8; e < d; e += 256 * 8)
        *reinterpret_cast<uint4*>(out + row * d + e) = *reinterpret_cast<const uint4*>(table + (size_t)id * d + e);
}

// ------------------------------------------------------------------ skinny GEMM (weight streaming)
// Y[M,N] = X[M,K] * W[N,K]^T (+ R[M,N]).  One 256-thread block owns 16 output columns; its 4
// waves split K four ways and each streams its quarter of the 16 W rows straight into MFMA B
// fragments (lane (n = l&15, g = l>>4) holds W[n0+n][k + 8g .. +7]: 16 B, k-contiguous), so W
// is read from HBM exactly once and never staged.  X fragments (A operand, same lane map over
// rows) are L2-resident re-reads.  MT = number of 16-row M tiles (M <= 16*MT); the four wave
// partials are summed through LDS.
// NW = 4 or 8 waves per block (8: the N <= 8192 projections, whose d/16 column blocks alone would leave one 4-wave block per CU -
// eight-way K split inside the block, no fp32 slabs for the consumer to sum).
// Small-M decoder-layer fusion of the two RMSNorm launches (a one-question step is a chain of ~7 launches per layer of which the
// two norms are 6.8 us each for 16 KB of data):
//   SSOUT  the d-wide projections (attention output / MLP down): Y = bf16(bf16(X W^T) + R) IS the new residual stream, and the block
//          also leaves the sum of squares of its 16 columns per row in ss_out[row][blockIdx.x] (summed by the consumer in a fixed
//          order: deterministic);
// The projections that read a normalised input (qkv, lm_head, gate/up) are skinny_normed_kernel: it takes the un-normalised
// residual stream H and a NormIn - the producer's per-block partial sums ss[row][0 .. nss) of the row's squares, the ln weights
// and eps - and normalises the rows once per block into LDS.
struct NormIn { const float* ss; int nss; const uint16_t* lnw; float eps; };

// What a lane streams of its weight row, behind one interface for the 16-bit and the 8-bit (e4m3 codes + a power-of-two scale per
// row, vdd_w8.h) forms of the few-row projections: `ld` fetches a register stage of U 32-deep k-steps at element kk of the wave's K
// slice, `ld1` the single k-step at element k (the slice's ragged last stage), `frag` turns one k-step of a stage into the MFMA B
// operand.  Both views feed the SAME fragments (up to the row's scale) to the same MFMAs in the same order; a SCALED view's kernel
// multiplies `wscale[row]` onto the fp32 sum before the epilogue's first rounding.
struct Rows16 {                        // [N][K] elements of the storage type
    typedef uint16_t code_t;
    typedef frag8_t stage_t;           // one k-step of a lane: W[n][k + 8 g .. + 7], 16 bytes
    static constexpr bool SCALED = false;
    const uint16_t* p;
    __device__ __forceinline__ Rows16(const uint16_t* W, size_t row, int K, int kbeg, int g) : p(W + row * K + kbeg + g * 8) {}
    template <class I, int U> __device__ __forceinline__ void ld(stage_t (&b)[U], int kk) const {
#pragma unroll
        for (int u = 0; u < U; ++u) b[u] = ld_w(p + (I)(kk + 32 * u));
    }
    template <class I> __device__ __forceinline__ stage_t ld1(int k) const { return ld_w(p + (I)k); }
    static __device__ __forceinline__ stage_t zero() { return stage_t{0, 0, 0, 0, 0, 0, 0, 0}; }
    static __device__ __forceinline__ frag8_t frag(stage_t s) { return s; }
};
struct RowsW8 {                        // [N][K] e4m3 codes in the storage order of include/vdd_hip.h ("8-bit weight rows"): the group
    typedef uint8_t code_t;            // of 64 elements that holds k-steps 2b and 2b + 1 is four 16-byte pieces, one per lane group g:
    typedef uint2 stage_t;             // its 8 codes of k-step 2b, then its 8 of k-step 2b + 1 - one k-step of a lane is 8 bytes
    static constexpr bool SCALED = true;
    const uint8_t* p;                  // the lane's piece of the group that holds the slice's first k-step
    int odd;                           // ... which is the group's second k-step (a K slice of an odd number of k-steps: K / 256 odd, 8 waves)
    __device__ __forceinline__ RowsW8(const uint8_t* W, size_t row, int K, int kbeg, int g)
        : p(W + row * K + (kbeg & ~63) + g * 16), odd(__builtin_amdgcn_readfirstlane((kbeg >> 5) & 1)) {}
    // a full stage (kk % 64 == 0): U / 2 loads of 16 bytes; from an odd start the two k-steps at the ends are 8-byte loads.  Every code
    // is read once either way
    template <class I, int U> __device__ __forceinline__ void ld(stage_t (&b)[U], int kk) const {
        static_assert(U % 2 == 0, "a 16-byte load is two k-steps");
        const uint8_t* q = p + (I)kk;
        if (!odd) {
#pragma unroll
            for (int j = 0; j < U / 2; ++j) { const uint4 v = *reinterpret_cast<const uint4*>(q + 64 * j); b[2 * j] = make_uint2(v.x, v.y); b[2 * j + 1] = make_uint2(v.z, v.w); }
        } else {
            b[0] = *reinterpret_cast<const uint2*>(q + 8);
#pragma unroll
            for (int j = 1; j < U / 2; ++j) { const uint4 v = *reinterpret_cast<const uint4*>(q + 64 * j); b[2 * j - 1] = make_uint2(v.x, v.y); b[2 * j] = make_uint2(v.z, v.w); }
            b[U - 1] = *reinterpret_cast<const uint2*>(q + 64 * (U / 2));
        }
    }
    template <class I> __device__ __forceinline__ stage_t ld1(int k) const {
        const int t = (k >> 5) + odd;                                                   // k-step counted from the first group
        return *reinterpret_cast<const uint2*>(p + (I)((t >> 1) * 64 + (t & 1) * 8));
    }
    static __device__ __forceinline__ stage_t zero() { return make_uint2(0u, 0u); }     // code 0x00 = +0
    static __device__ __forceinline__ frag8_t frag(stage_t s) { return __builtin_bit_cast(frag8_t, w8_widen(s)); }
};

// two elements (packed in a dword) -> rnd(rnd(h * rstd) * g) with the hardware's RNE pack conversion (v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32)
__device__ __forceinline__ uint32_t norm_pair(uint32_t hv, uint32_t gv, float rstd) {
    const uint32_t nb = cvt_pk(lo(hv) * rstd, hi(hv) * rstd);
    return cvt_pk(lo(nb) * lo(gv), hi(nb) * hi(gv));
}
__device__ __forceinline__ uint4 norm_chunk(uint4 a, uint4 w, float rstd) {
    return make_uint4(norm_pair(a.x, w.x, rstd), norm_pair(a.y, w.y, rstd), norm_pair(a.z, w.z, rstd), norm_pair(a.w, w.w, rstd));
}

// Persistent form of the weight-streaming projections for a NORMALISED input: a block normalises the (<= 16) rows of H ONCE into LDS
// - bf16(bf16(h * rstd) * ln_w[k]), the roundings of rmsnorm_kernel - behind its first batch of W loads, then walks its column
// blocks (blockIdx.x, + gridDim.x, ...) with the A fragments read from LDS.  (Normalising per column block - in every one of the
// 768 - 2000 blocks of the plain kernels - costs more VALU time than the two RMSNorm launches it replaces: 6.2 vs 3.4 ms per
// one-question step.)  LDS image: row r at byte 2 K r, its 16-byte chunk q at slot q ^ (r & 15): a ds_read_b128 is served in four
// 16-lane groups ({0-3, 12-15, 20-27}, ...: 16 DISTINCT rows at two adjacent chunks) and the XOR puts those on 16 distinct slots of the
// 256-byte bank row (a padded stride of 2 K + 64 left them 2-way conflicted: 16 rows cost 33 us where 2 rows - broadcast - cost 21).
// SWIGLU: a column block is 8 features (gate rows | up rows of W = [Wg; Wu]) with the SiLU * mul epilogue of skinny_swiglu_kernel.
template <int NW, bool SWIGLU, int RMAX, class WV = Rows16>   // RMAX: M rounded up to 2 / 4 / 8 / 16 (the prologue is straight-line code over RMAX rows)
__global__ void __launch_bounds__(NW * 64) skinny_normed_kernel(const uint16_t* __restrict__ Hs, const typename WV::code_t* __restrict__ W,
                                                               uint16_t* __restrict__ Y, int M, int N, int K, long long ldh,
                                                               long long ldy, NormIn ni, int n_cb, const float* __restrict__ wscale) {
    extern __shared__ __attribute__((aligned(16))) unsigned char xs[];           // [M][2 K] bytes, chunk-swizzled
    __shared__ float part2[2][NW][64][4];                                         // double-buffered: ONE barrier per column block
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ln = lane & 15, g = lane >> 4;
    const int kq = K / NW, kbeg = wave * kq;
    const int rstride = 2 * K;
    constexpr int U = 8;
    // a wave's K slice as nb batches of U 32-deep k-steps; a ragged last batch (K = 5120 over 8 waves: 640 = 2 batches + 128) loads
    // from clamped addresses and multiplies the k-steps beyond the slice by a zero W fragment
    const int nb = (kq + 32 * U - 1) / (32 * U);
    const bool ragged = (kq % (32 * U)) != 0;
    typedef typename WV::stage_t wstage_t;
    auto wptr = [&](int cb) {
        if constexpr (SWIGLU) { int f = cb * 8 + (ln & 7); if (f >= N) f = N - 1; return WV(W, (size_t)(ln < 8 ? 0 : N) + f, K, kbeg, g); }
        else { int nrow = cb * 16 + ln; if (nrow >= N) nrow = N - 1; return WV(W, (size_t)nrow, K, kbeg, g); }
    };
    wstage_t b0[U], b1[U];
    auto ldw = [&](wstage_t (&b)[U], const WV& wp, int i) {
        const int kk = i * 32 * U;
        if (ragged && i == nb - 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) b[u] = wp.template ld1<int>(kk + 32 * u < kq ? kk + 32 * u : kk);
        } else {
            wp.template ld<int>(b, kk);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    int cb = blockIdx.x;
    WV wp = wptr(cb < n_cb ? cb : 0);
    if (nb > 0) ldw(b0, wp, 0);                                                // the weight stream starts before anything else:
    bool b1_ahead = false;                                                     // BOTH register stages of the first column block are
    if (nb > 1) { ldw(b1, wp, 1); b1_ahead = true; }                           // in flight under the normalisation prologue
    // ---- normalise the rows into LDS (once per block).  Sum of squares of a row = its nss per-block partials: thread t takes
    // partials t, t + NT, ... (one load per row for d <= 4096), butterfly over the wave, the NW wave sums in a fixed tree: one
    // memory round trip for all rows together and deterministic.  (A per-thread loop over the partials of a row is a chain of
    // dependent round trips: 10 us per launch.)
    __shared__ float red[NW][16];
    {
        // everything the normalisation reads goes out in ONE memory round trip, as STRAIGHT-LINE code: the per-block partial sums of
        // all rows, the ln weights and the first RB rows of H (further row batches: one round trip each).  Loads are never
        // predicated - a row / chunk / partial that does not exist is read at a clamped, valid address and dropped: a load inside an
        // `if` or a run-time loop ends in its own s_waitcnt, which made the prologue a chain of M round trips (16 rows: 12 us).
        constexpr int NT = NW * 64, CMAX = 16 / NW, RB = RMAX < 16 / CMAX ? RMAX : 16 / CMAX, PMAX = 512 / NT;   // K <= 8192, nss <= 512
        float pv[RMAX][PMAX];
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            const int rc = r < M ? r : M - 1;
#pragma unroll
            for (int q = 0; q < PMAX; ++q) {
                const int i = tid + q * NT;
                pv[r][q] = ni.ss[(size_t)rc * ni.nss + (i < ni.nss ? i : 0)];
            }
        }
        uint4 gw[CMAX], hv[RB][CMAX];
        auto ld_rows = [&](int r0) {
#pragma unroll
            for (int j = 0; j < RB; ++j) {
                const int rc = r0 + j < M ? r0 + j : M - 1;
#pragma unroll
                for (int c = 0; c < CMAX; ++c) {
                    const int e = (c * NT + tid) * 8;
                    hv[j][c] = *reinterpret_cast<const uint4*>(Hs + (size_t)rc * ldh + (e < K ? e : 0));
                }
            }
        };
#pragma unroll
        for (int c = 0; c < CMAX; ++c) { const int e = (c * NT + tid) * 8; gw[c] = *reinterpret_cast<const uint4*>(ni.lnw + (e < K ? e : 0)); }
        ld_rows(0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < PMAX; ++q) v += (tid + q * NT < ni.nss) ? pv[r][q] : 0.f;
            const float sw = wave_sum(v);
            if (lane == 0) red[wave][r] = sw;
        }
        __syncthreads();
        for (int r0 = 0; r0 < M; r0 += RB) {
            if (r0 > 0) { ld_rows(r0); __builtin_amdgcn_sched_barrier(0); }
#pragma unroll
            for (int j = 0; j < RB; ++j) {
                const int r = r0 + j;
                const float tot = wave_partial_sum<NW>(&red[0][r & 15], 16);
                const float rstd = rsqrtf(tot / (float)K + ni.eps);
#pragma unroll
                for (int c = 0; c < CMAX; ++c) {
                    const int e = (c * NT + tid) * 8;
                    const uint4 nv = norm_chunk(hv[j][c], gw[c], rstd);
                    if (r < M && e < K) *reinterpret_cast<uint4*>(xs + (size_t)r * rstride + ((e * 2) ^ ((r & 15) << 4))) = nv;
                }
            }
        }
    }
    __syncthreads();
    int rr = ln; if (rr >= M) rr = M - 1;
    const unsigned char* xrow = xs + (size_t)rr * rstride;
    const int xk0 = (kbeg + g * 8) * 2, xsw = (rr & 15) << 4;
    auto xfrag = [&](int k) { return *reinterpret_cast<const frag8_t*>(xrow + ((xk0 + k * 2) ^ xsw)); };
    auto mm = [&](const wstage_t (&b)[U], int i, f32x4_t& acc) {
        const int kk = i * 32 * U;
        if (ragged && i == nb - 1) {
            const frag8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = kk + 32 * u < kq;
                acc = mfma16(xfrag(in ? kk + 32 * u : kk), in ? WV::frag(b[u]) : zero, acc);
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u)
                acc = mfma16(xfrag(kk + 32 * u), WV::frag(b[u]), acc);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    int pbuf = 0;
    for (; cb < n_cb; cb += gridDim.x) {
        f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
        int it = 0;
        for (; it + 2 <= nb; it += 2) {
            if (!b1_ahead) ldw(b1, wp, it + 1);
            b1_ahead = false;
            mm(b0, it, acc);
            if (it + 2 < nb) ldw(b0, wp, it + 2);
            mm(b1, it + 1, acc);
        }
        if (it < nb) mm(b0, it, acc);
        const int cb_next = cb + gridDim.x;
        const WV wp_next = wptr(cb_next < n_cb ? cb_next : cb);
        // BOTH register stages of the next column block go out before the barrier: the weight stream does not drain while the block
        // meets.  The partial sums alternate between two LDS buffers: the waves that do not finish the tile go straight on to the
        // next one (a buffer is rewritten two column blocks later, behind the barrier in between).
        if (cb_next < n_cb && nb > 0) { ldw(b0, wp_next, 0); if (nb > 1) { ldw(b1, wp_next, 1); b1_ahead = true; } }
        float (*part)[64][4] = part2[pbuf];
        pbuf ^= 1;
        // 8-bit weights: the power-of-two scale of the finishing thread's output row(s), fetched ahead of the barrier
        float sc0 = 1.f, sc1 = 1.f;
        if constexpr (WV::SCALED) {
            if constexpr (SWIGLU) { int f = cb * 8 + (tid & 7); if (f >= N) f = N - 1; sc0 = wscale[f]; sc1 = wscale[N + f]; }
            else { int col = cb * 16 + ln; if (col >= N) col = N - 1; sc0 = wscale[col]; }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) part[wave][lane][r] = acc[r];
        __syncthreads();
        if constexpr (SWIGLU) {
            if (tid < 128) {           // C map: col = lane & 15, row = (lane >> 4) * 4 + r.  (row = tid / 8, feature = tid % 8)
                const int row = tid >> 3, c = tid & 7;
                if (row < M && cb * 8 + c < N) {
                    const int lg = (row >> 2) * 16 + c, lu = lg + 8, q = row & 3;
                    float gs = 0.f, us = 0.f;           // wave_partial_sum's tree, written out: through the helper this site's LDS address
                    gs = (part[0][lg][q] + part[1][lg][q]) + (part[2][lg][q] + part[3][lg][q]);       // arithmetic compiles to other instructions
                    us = (part[0][lu][q] + part[1][lu][q]) + (part[2][lu][q] + part[3][lu][q]);
                    if constexpr (NW == 8) { gs += (part[4][lg][q] + part[5][lg][q]) + (part[6][lg][q] + part[7][lg][q]);
                                             us += (part[4][lu][q] + part[5][lu][q]) + (part[6][lu][q] + part[7][lu][q]); }
                    if constexpr (WV::SCALED) { gs *= sc0; us *= sc1; }
                    Y[(size_t)row * ldy + cb * 8 + c] = swiglu_out(gs, us);
                }
            }
        } else {
            if (wave == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = g * 4 + r, col = cb * 16 + ln;
                    float sacc = wave_partial_sum<NW>(&part[0][lane][r], 64 * 4);
                    if constexpr (WV::SCALED) sacc *= sc0;
                    if (row < M && col < N) Y[(size_t)row * ldy + col] = (uint16_t)f2e(sacc);
                }
            }
        }
        wp = wp_next;
    }
}

template <int MT, int NW, bool SSOUT = false, class WV = Rows16>
__global__ void __launch_bounds__(NW * 64) skinny_gemm_kernel(const uint16_t* __restrict__ X, const typename WV::code_t* __restrict__ W,
                                                             const uint16_t* __restrict__ R, uint16_t* __restrict__ Y,
                                                             float* __restrict__ Yslab, int M, int N, int K, long long ldx,
                                                             long long ldr, long long ldy, float* __restrict__ ss_out,
                                                             const float* __restrict__ wscale) {
    __shared__ float part[NW][MT][64][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * 16;
    const int ln = lane & 15, g = lane >> 4;
    // gridDim.y > 1: split-K across blocks as well; slice s writes the fp32 slab Yslab[s][M][N], summed by the RMSNorm that consumes it
    const int kq = K / (NW * (int)gridDim.y);
    const int kbeg = ((int)blockIdx.y * NW + wave) * kq;
    int nrow = n0 + ln; if (nrow >= N) nrow = N - 1;
    const WV wp(W, (size_t)nrow, K, kbeg, g);
    typedef typename WV::stage_t wstage_t;
    const uint16_t* xp[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) { int r = t * 16 + ln; if (r >= M) r = M - 1; xp[t] = X + (size_t)r * ldx + kbeg + g * 8; }
    f32x4_t acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // Two register stages: the loads of batch i + 1 (8 x 16 B of W per lane) go out before the MFMAs of batch i, so a wave's K
    // slice (1,024 - 2,752 elements = 4 - 10 batches) costs ONE memory round trip plus streaming instead of one per batch (a
    // one-question step is a chain of these launches: see DESIGN.md section 5).  Same MFMAs in the same order.
    constexpr int U = MT > 2 ? 4 : 8;                  // k-steps per register stage (33 - 64 rows: 4, so that TWO stages of 16 - 20 fragments fit)
    const int nit = kq / (32 * U);
    wstage_t b0[U], b1[U];
    frag8_t a0[U][MT], a1[U][MT];
    auto ld = [&](wstage_t (&b)[U], frag8_t (&a)[U][MT], int kk) {
        wp.template ld<size_t>(b, kk);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < MT; ++t) a[u][t] = *reinterpret_cast<const frag8_t*>(xp[t] + kk + 32 * u);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto mm = [&](const wstage_t (&b)[U], const frag8_t (&a)[U][MT]) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < MT; ++t) acc[t] = mfma16(a[u][t], WV::frag(b[u]), acc[t]);
        __builtin_amdgcn_sched_barrier(0);
    };
    uint16_t rpre[4] = {0, 0, 0, 0};                    // MT == 1: wave 0's residual entries, fetched under the weight stream
    {   // Two register stages at every row count (MT = 2: 2 x (32 + 64) registers; MT = 3 / 4 with U = 4: 2 x (16 + 64)).  A single stage
        // paid one memory round trip per batch - 11 in a row for the down projection's 2,752-deep wave slices: 33.3 -> 26.6 us for its
        // 90 MB at 17 rows, 34.3 -> 33.8 at 32; the attention output at 40 / 48 / 64 rows 19.5 / 20.7 / 23.5 -> 17.1 / 18.3 / 20.9 us.
        // (Eight waves per block with two stages at 17 - 32 rows: 29.6 / 37.6 - slower; tools/skinny_crossover_probe.py.)
        if (nit > 0) ld(b0, a0, 0);
        if (MT == 1 && R != nullptr && wave == 0 && Yslab == nullptr) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { const int row = g * 4 + r, col = n0 + ln; if (row < M && col < N) rpre[r] = R[(size_t)row * ldr + col]; }
        }
        int it = 0;
        for (; it + 2 <= nit; it += 2) {
            ld(b1, a1, (it + 1) * 32 * U);
            mm(b0, a0);
            if (it + 2 < nit) ld(b0, a0, (it + 2) * 32 * U);
            mm(b1, a1);
        }
        if (it < nit) mm(b0, a0);
    }
    // the K slice's remainder (K = 11008 over 8 waves: 1376 = 5 batches + 96): ONE more batch whose loads all go out together, the
    // k-steps beyond the slice with a zero W fragment (+0 to the accumulators; X is read at a clamped, valid address) - a loop of
    // load -> MFMA is a chain of memory round trips at the end of every block
    const int krem = nit * 32 * U;
    if (krem < kq) {
        const wstage_t zero = WV::zero();
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kk = krem + 32 * u, kc = kk < kq ? kk : krem;
            b0[u] = wp.template ld1<size_t>(kc);
#pragma unroll
            for (int t = 0; t < MT; ++t) a0[u][t] = *reinterpret_cast<const frag8_t*>(xp[t] + kc);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u) if (krem + 32 * u >= kq) b0[u] = zero;
        mm(b0, a0);
    }
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[wave][t][lane][r] = acc[t][r];
    float sc = 1.f;                                     // 8-bit weights: the power-of-two scale of this lane's output column
    if constexpr (WV::SCALED) sc = wscale[nrow];
    __syncthreads();
    // C/D map of 16x16x32: col = lane & 15, row = (lane >> 4) * 4 + r.  Wave w finishes tile(s) t = w, w+4, ...
    for (int t = wave; t < MT; t += NW) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = t * 16 + g * 4 + r, col = n0 + ln;
            float s = wave_partial_sum<NW>(&part[0][t][lane][r], MT * 64 * 4);
            if constexpr (WV::SCALED) s *= sc;
            float sq = 0.f;
            if (row < M && col < N) {
                if (Yslab != nullptr) { Yslab[((size_t)blockIdx.y * M + row) * N + col] = s; continue; }
                float o = e2f(f2e(s));
                if (R != nullptr) o = o + e2f(MT == 1 ? rpre[r] : R[(size_t)row * ldr + col]);
                const uint32_t ob = f2e(o);
                Y[(size_t)row * ldy + col] = (uint16_t)ob;
                if constexpr (SSOUT) { const float h = e2f(ob); sq = h * h; }
            }
            if constexpr (SSOUT) {      // the 16 lanes ln = 0..15 of a lane group hold the block's 16 columns of one row
                sq += __shfl_xor(sq, 1); sq += __shfl_xor(sq, 2); sq += __shfl_xor(sq, 4); sq += __shfl_xor(sq, 8);
                if (ln == 0 && row < M) ss_out[(size_t)row * gridDim.x + blockIdx.x] = sq;
            }
        }
    }
}

// ------------------------------------------------------------------ skinny gate/up GEMM with the SwiGLU epilogue
// act[M,F] = silu(X Wg^T) * (X Wu^T), W = [Wg; Wu] ([2F, K]).  The 16 MFMA columns of a block are 8 gate columns
// (B-fragment lanes ln < 8 -> row f0 + ln) and the 8 matching up columns (ln >= 8 -> row F + f0 + ln - 8), so the
// epilogue finds gate and up of one feature in the same LDS tile: no [M, 2F] round trip and no silu_mul launch.
// Rounding as the unfused pair: gate, up -> bf16; silu(gate) -> bf16; product -> bf16.
// WV = RowsW8: W holds codes, wscale the 2F row scales (gate rows first); gate and up take their own scale before the first rounding.
template <class WV = Rows16>
__global__ void __launch_bounds__(256) skinny_swiglu_kernel(const uint16_t* __restrict__ X, const typename WV::code_t* __restrict__ W,
                                                            uint16_t* __restrict__ A, int M, int F, int K, long long ldx,
                                                            const float* __restrict__ wscale) {
    __shared__ float part[4][64][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f0 = blockIdx.x * 8;
    const int ln = lane & 15, g = lane >> 4;
    const int kq = K / 4, kbeg = wave * kq;
    int f = f0 + (ln & 7); if (f >= F) f = F - 1;
    const WV wp(W, (size_t)(ln < 8 ? 0 : F) + f, K, kbeg, g);
    typedef typename WV::stage_t wstage_t;
    int r = ln; if (r >= M) r = M - 1;
    const uint16_t* xp = X + (size_t)r * ldx + kbeg + g * 8;
    f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
    constexpr int U = 8;             // two register stages, as in skinny_gemm_kernel
    const int nit = kq / (32 * U);
    wstage_t b0[U], b1[U];
    frag8_t a0[U], a1[U];
    auto ld = [&](wstage_t (&b)[U], frag8_t (&a)[U], int kk) {
        wp.template ld<size_t>(b, kk);
#pragma unroll
        for (int u = 0; u < U; ++u) a[u] = *reinterpret_cast<const frag8_t*>(xp + kk + 32 * u);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto mm = [&](const wstage_t (&b)[U], const frag8_t (&a)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) acc = mfma16(a[u], WV::frag(b[u]), acc);
        __builtin_amdgcn_sched_barrier(0);
    };
    if (nit > 0) ld(b0, a0, 0);
    int it = 0;
    for (; it + 2 <= nit; it += 2) {
        ld(b1, a1, (it + 1) * 32 * U);
        mm(b0, a0);
        if (it + 2 < nit) ld(b0, a0, (it + 2) * 32 * U);
        mm(b1, a1);
    }
    if (it < nit) mm(b0, a0);
    int k = nit * 32 * U;
    for (; k < kq; k += 32) {
        const frag8_t a = *reinterpret_cast<const frag8_t*>(xp + k);
        acc = mfma16(a, WV::frag(wp.template ld1<size_t>(k)), acc);
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) part[wave][lane][rr] = acc[rr];
    float sc0 = 1.f, sc1 = 1.f;      // 8-bit weights: the power-of-two scales of the finishing thread's gate and up rows
    if constexpr (WV::SCALED) { int fc = f0 + (tid & 7); if (fc >= F) fc = F - 1; sc0 = wscale[fc]; sc1 = wscale[F + fc]; }
    __syncthreads();
    // C map: col = lane & 15, row = (lane >> 4) * 4 + rr.  Threads 0..127: (row = tid / 8, feature = tid % 8)
    if (tid < 128) {
        const int row = tid >> 3, c = tid & 7;
        if (row < M && f0 + c < F) {
            const int lg = (row >> 2) * 16 + c, lu = lg + 8, rr = row & 3;
            float gs = wave_partial_sum<4>(&part[0][lg][rr], 64 * 4), us = wave_partial_sum<4>(&part[0][lu][rr], 64 * 4);
            if constexpr (WV::SCALED) { gs *= sc0; us *= sc1; }
            A[(size_t)row * F + f0 + c] = swiglu_out(gs, us);
        }
    }
}

// ------------------------------------------------------------------ weight streaming for 17 - 64 rows
// A few dozen rows in flight (an 8-GPU split of config #3 leaves 34 rows per rank; config #5 on 4 GPUs ~190): too many for the
// 16-column blocks above - every block re-reads ALL of X from L2, 4 X fragments per W fragment at 64 rows, and that traffic (400 MB
// for the qkv projection against 100 MB of weights) is what the launch then moves - and too few for the MFMA GEMM, whose 64 x 256
// tiles cover a fraction of the CUs and pay a serial stream-K fix-up (30 - 43 us per projection whatever M <= 64).
// Here a block owns 32 output columns - two MFMA column tiles sharing every X fragment - its NW waves split K, and the loads of
// batch i + 1 (U k-steps: 2 U W fragments + MT U X fragments per lane) are in flight under the MFMAs of batch i.  W is still read
// from HBM exactly once.  SWIGLU: the two column tiles are 16 gate columns and the 16 matching up columns of W = [Wg; Wu], so the
// epilogue pairs them in registers: act = rnd(rnd(silu(rnd(gate))) * rnd(up)), the rounding points of the unfused pair.
template <int MT, int NW, bool SWIGLU>
__global__ void __launch_bounds__(NW * 64) skinny_wide_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ W,
                                                             const uint16_t* __restrict__ R, uint16_t* __restrict__ Y, int M, int N, int K,
                                                             long long ldx, long long ldr, long long ldy) {
    extern __shared__ __attribute__((aligned(16))) float wide_part[];            // [NW][MT][2][64][4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ln = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * (SWIGLU ? 16 : 32);                               // SWIGLU: N = F features, 16 per block
    const int kq = K / NW, kbeg = wave * kq;
    const uint16_t* wp[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        int row = SWIGLU ? n0 + ln : n0 + 16 * c + ln;
        if (row >= N) row = N - 1;
        wp[c] = W + ((size_t)(SWIGLU && c == 1 ? N : 0) + row) * K + kbeg + g * 8;
    }
    const uint16_t* xp[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) { int r = t * 16 + ln; if (r >= M) r = M - 1; xp[t] = X + (size_t)r * ldx + kbeg + g * 8; }
    f32x4_t acc[MT][2];
#pragma unroll
    for (int t = 0; t < MT; ++t) { acc[t][0] = f32x4_t{0.f, 0.f, 0.f, 0.f}; acc[t][1] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
    constexpr int U = MT >= 4 ? 2 : 4;           // k-steps per register stage (64 rows: 2 x (2 + 4) fragments x 2 stages + 32 accumulators fill the file)
    const int nit = kq / (32 * U);
    frag8_t b0[U][2], a0[U][MT], b1[U][2], a1[U][MT];
    auto ld = [&](frag8_t (&b)[U][2], frag8_t (&a)[U][MT], int kk) {
#pragma unroll
        for (int u = 0; u < U; ++u) { b[u][0] = ld_w(wp[0] + kk + 32 * u); b[u][1] = ld_w(wp[1] + kk + 32 * u); }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < MT; ++t) a[u][t] = *reinterpret_cast<const frag8_t*>(xp[t] + kk + 32 * u);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto mm = [&](const frag8_t (&b)[U][2], const frag8_t (&a)[U][MT]) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                acc[t][0] = mfma16(a[u][t], b[u][0], acc[t][0]);
                acc[t][1] = mfma16(a[u][t], b[u][1], acc[t][1]);
            }
        __builtin_amdgcn_sched_barrier(0);
    };
    if (nit > 0) ld(b0, a0, 0);
    int it = 0;
    for (; it + 2 <= nit; it += 2) {
        ld(b1, a1, (it + 1) * 32 * U);
        mm(b0, a0);
        if (it + 2 < nit) ld(b0, a0, (it + 2) * 32 * U);
        mm(b1, a1);
    }
    if (it < nit) mm(b0, a0);
    const int krem = nit * 32 * U;
    if (krem < kq) {            // the slice's ragged tail (11008 / 8 = 1376 = 10 batches + 96): one more batch, k-steps beyond it with zero W
        const frag8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kk = krem + 32 * u, kc = kk < kq ? kk : krem;
            b0[u][0] = ld_w(wp[0] + kc); b0[u][1] = ld_w(wp[1] + kc);
#pragma unroll
            for (int t = 0; t < MT; ++t) a0[u][t] = *reinterpret_cast<const frag8_t*>(xp[t] + kc);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u) if (krem + 32 * u >= kq) { b0[u][0] = zero; b0[u][1] = zero; }
        mm(b0, a0);
    }
    auto part = [&](int w, int t, int c) { return wide_part + ((((size_t)w * MT + t) * 2 + c) * 64) * 4; };
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int c = 0; c < 2; ++c) *reinterpret_cast<f32x4_t*>(part(wave, t, c) + lane * 4) = acc[t][c];
    __syncthreads();
    // C/D map of 16x16x32: col = lane & 15, row = (lane >> 4) * 4 + r.  The NW partials of an entry are added in wave order (fixed).
    auto total = [&](int t, int c) {
        f32x4_t s = *reinterpret_cast<const f32x4_t*>(part(0, t, c) + lane * 4);
#pragma unroll
        for (int w = 1; w < NW; ++w) { const f32x4_t v = *reinterpret_cast<const f32x4_t*>(part(w, t, c) + lane * 4); s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3]; }
        return s;
    };
    if constexpr (SWIGLU) {
        for (int t = wave; t < MT; t += NW) {
            const f32x4_t gs = total(t, 0), us = total(t, 1);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = t * 16 + g * 4 + r, col = n0 + ln;
                if (row < M && col < N) Y[(size_t)row * ldy + col] = swiglu_out(gs[r], us[r]);
            }
        }
    } else {
        for (int tc = wave; tc < MT * 2; tc += NW) {
            const int t = tc >> 1, c = tc & 1;
            const f32x4_t sv = total(t, c);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = t * 16 + g * 4 + r, col = n0 + 16 * c + ln;
                if (row < M && col < N) {
                    float o = e2f(f2e(sv[r]));
                    if (R != nullptr) o = o + e2f(R[(size_t)row * ldr + col]);
                    Y[(size_t)row * ldy + col] = (uint16_t)f2e(o);
                }
            }
        }
    }
}

// The 8-bit sibling of skinny_wide_kernel (without the residual): W holds e4m3 codes behind the RowsW8 view - a stage of U = 2 / 4 k-steps
// is one / two 16-byte loads per column tile; K % 256 == 0 over four waves starts every wave slice on a group of 64 - and wscale the row
// scales ([2N] for SWIGLU, gate rows first), multiplied onto the summed partials of each column tile before the first rounding.  The same
// MFMAs in the same order as the 16-bit kernel.  A sibling and not a template parameter of it: behind the Rows16 view the 16-bit
// kernel's address arithmetic compiled to another instruction order.
template <int MT, int NW, bool SWIGLU>
__global__ void __launch_bounds__(NW * 64) skinny_wide_w8_kernel(const uint16_t* __restrict__ X, const uint8_t* __restrict__ W,
                                                                uint16_t* __restrict__ Y, int M, int N, int K, long long ldx, long long ldy,
                                                                const float* __restrict__ wscale) {
    typedef RowsW8 WV;
    extern __shared__ __attribute__((aligned(16))) float wide_part[];            // [NW][MT][2][64][4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ln = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * (SWIGLU ? 16 : 32);                               // SWIGLU: N = F features, 16 per block
    const int kq = K / NW, kbeg = wave * kq;
    auto wrow = [&](int c) {                                                      // this lane's W row of column tile c
        int row = SWIGLU ? n0 + ln : n0 + 16 * c + ln;
        if (row >= N) row = N - 1;
        return (size_t)(SWIGLU && c == 1 ? N : 0) + row;
    };
    const WV wp[2] = {WV(W, wrow(0), K, kbeg, g), WV(W, wrow(1), K, kbeg, g)};
    typedef typename WV::stage_t wstage_t;
    const uint16_t* xp[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) { int r = t * 16 + ln; if (r >= M) r = M - 1; xp[t] = X + (size_t)r * ldx + kbeg + g * 8; }
    f32x4_t acc[MT][2];
#pragma unroll
    for (int t = 0; t < MT; ++t) { acc[t][0] = f32x4_t{0.f, 0.f, 0.f, 0.f}; acc[t][1] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
    constexpr int U = MT >= 4 ? 2 : 4;           // k-steps per register stage (64 rows: 2 x (2 + 4) fragments x 2 stages + 32 accumulators fill the file)
    const int nit = kq / (32 * U);
    wstage_t b0[2][U], b1[2][U];
    frag8_t a0[U][MT], a1[U][MT];
    auto ld = [&](wstage_t (&b)[2][U], frag8_t (&a)[U][MT], int kk) {
        wp[0].template ld<int>(b[0], kk); wp[1].template ld<int>(b[1], kk);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < MT; ++t) a[u][t] = *reinterpret_cast<const frag8_t*>(xp[t] + kk + 32 * u);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto mm = [&](const wstage_t (&b)[2][U], const frag8_t (&a)[U][MT]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const frag8_t w0 = WV::frag(b[0][u]), w1 = WV::frag(b[1][u]);
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                acc[t][0] = mfma16(a[u][t], w0, acc[t][0]);
                acc[t][1] = mfma16(a[u][t], w1, acc[t][1]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    if (nit > 0) ld(b0, a0, 0);
    int it = 0;
    for (; it + 2 <= nit; it += 2) {
        ld(b1, a1, (it + 1) * 32 * U);
        mm(b0, a0);
        if (it + 2 < nit) ld(b0, a0, (it + 2) * 32 * U);
        mm(b1, a1);
    }
    if (it < nit) mm(b0, a0);
    const int krem = nit * 32 * U;
    if (krem < kq) {            // the slice's ragged tail (11008 / 8 = 1376 = 10 batches + 96): one more batch, k-steps beyond it with zero W
        const wstage_t zero = WV::zero();
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kk = krem + 32 * u, kc = kk < kq ? kk : krem;
            b0[0][u] = wp[0].template ld1<int>(kc); b0[1][u] = wp[1].template ld1<int>(kc);
#pragma unroll
            for (int t = 0; t < MT; ++t) a0[u][t] = *reinterpret_cast<const frag8_t*>(xp[t] + kc);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u) if (krem + 32 * u >= kq) { b0[0][u] = zero; b0[1][u] = zero; }
        mm(b0, a0);
    }
    auto part = [&](int w, int t, int c) { return wide_part + ((((size_t)w * MT + t) * 2 + c) * 64) * 4; };
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int c = 0; c < 2; ++c) *reinterpret_cast<f32x4_t*>(part(wave, t, c) + lane * 4) = acc[t][c];
    const float scw[2] = {wscale[wrow(0)], wscale[wrow(1)]};                     // the power-of-two scales of this lane's column in either tile
    __syncthreads();
    // C/D map of 16x16x32: col = lane & 15, row = (lane >> 4) * 4 + r.  The NW partials of an entry are added in wave order (fixed).
    auto total = [&](int t, int c) {
        f32x4_t s = *reinterpret_cast<const f32x4_t*>(part(0, t, c) + lane * 4);
#pragma unroll
        for (int w = 1; w < NW; ++w) { const f32x4_t v = *reinterpret_cast<const f32x4_t*>(part(w, t, c) + lane * 4); s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3]; }
        return s;
    };
    if constexpr (SWIGLU) {
        for (int t = wave; t < MT; t += NW) {
            f32x4_t gs = total(t, 0), us = total(t, 1);
            gs[0] *= scw[0]; gs[1] *= scw[0]; gs[2] *= scw[0]; gs[3] *= scw[0];
            us[0] *= scw[1]; us[1] *= scw[1]; us[2] *= scw[1]; us[3] *= scw[1];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = t * 16 + g * 4 + r, col = n0 + ln;
                if (row < M && col < N) Y[(size_t)row * ldy + col] = swiglu_out(gs[r], us[r]);
            }
        }
    } else {
        for (int tc = wave; tc < MT * 2; tc += NW) {
            const int t = tc >> 1, c = tc & 1;
            f32x4_t sv = total(t, c);
            const float sc = c ? scw[1] : scw[0];
            sv[0] *= sc; sv[1] *= sc; sv[2] *= sc; sv[3] *= sc;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = t * 16 + g * 4 + r, col = n0 + 16 * c + ln;
                if (row < M && col < N) Y[(size_t)row * ldy + col] = (uint16_t)f2e(sv[r]);
            }
        }
    }
}

// ------------------------------------------------------------------ launch helpers of the weight-streaming entries
// compute units of the current device (256 where it cannot be asked), asked once per process
static int cu_count() {
    static int n_cu = 0;
    if (n_cu == 0) { int dev = 0, n = 0; n_cu = (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256; }
    return n_cu;
}

// Eight waves per 16-column block (K split eight ways inside the block) are ONE resident block per CU: right when the column blocks
// fill the chip in whole rounds (N = 4096: 256 blocks on 256 CUs).  N = 5120 (LLaVA-1.5-13B) is 320 blocks - a second round for a
// quarter of the chip, 0.62 of the stream rate (o-projection 23.9 us for 52 MB, down 48.9 us for 141 MB at 12 rows); four-wave
// blocks are small enough for three per CU, so all 320 stream at once.
static bool eight_wave_blocks(int N) {
    const int blocks = (N + 15) / 16;
    return blocks <= cu_count() || blocks % cu_count() == 0;
}

// skinny_wide_kernel for 17 - 64 rows: 32 columns per block, or (SWIGLU: N = F, W = [Wg; Wu]) 16 features = gate + up tiles
template <bool SWIGLU>
static void wide_launch(const uint16_t* x, const uint16_t* w, const uint16_t* r, uint16_t* y, int M, int N, int K, int64_t ldx, int64_t ldr,
                        int64_t ldy, hipStream_t st) {
    const int mt = (M + 15) / 16;
    const dim3 g2(SWIGLU ? (N + 15) / 16 : (N + 31) / 32);
#define VDD_WIDE(MT, NW, SWIGLU)                                                                                                       \
    do {                                                                                                                               \
        constexpr int smem = NW * MT * 2 * 64 * 4 * (int)sizeof(float);                                                                \
        static bool attr = false;                                                                                                      \
        if (!attr) { (void)hipFuncSetAttribute((const void*)skinny_wide_kernel<MT, NW, SWIGLU>, hipFuncAttributeMaxDynamicSharedMemorySize, smem); attr = true; } \
        hipLaunchKernelGGL((skinny_wide_kernel<MT, NW, SWIGLU>), g2, dim3(NW * 64), smem, st, x, w, r, y, M, N, K, (long long)ldx, (long long)ldr, (long long)ldy); \
    } while (0)
    if (mt == 2) VDD_WIDE(2, 4, SWIGLU); else if (mt == 3) VDD_WIDE(3, 4, SWIGLU); else VDD_WIDE(4, 4, SWIGLU);
#undef VDD_WIDE
}

// ... and its 8-bit sibling
template <bool SWIGLU>
static void wide_w8_launch(const uint16_t* x, const uint8_t* w, const float* wscale, uint16_t* y, int M, int N, int K, int64_t ldx, int64_t ldy,
                           hipStream_t st) {
    const int mt = (M + 15) / 16;
    const dim3 g2(SWIGLU ? (N + 15) / 16 : (N + 31) / 32);
#define VDD_WIDE_W8(MT, NW, SWIGLU)                                                                                                    \
    do {                                                                                                                               \
        constexpr int smem = NW * MT * 2 * 64 * 4 * (int)sizeof(float);                                                                \
        static bool attr = false;                                                                                                      \
        if (!attr) { (void)hipFuncSetAttribute((const void*)skinny_wide_w8_kernel<MT, NW, SWIGLU>, hipFuncAttributeMaxDynamicSharedMemorySize, smem); attr = true; } \
        hipLaunchKernelGGL((skinny_wide_w8_kernel<MT, NW, SWIGLU>), g2, dim3(NW * 64), smem, st, x, w, y, M, N, K, (long long)ldx, (long long)ldy, wscale); \
    } while (0)
    if (mt == 2) VDD_WIDE_W8(2, 4, SWIGLU); else if (mt == 3) VDD_WIDE_W8(3, 4, SWIGLU); else VDD_WIDE_W8(4, 4, SWIGLU);
#undef VDD_WIDE_W8
}

// the d-wide projections of the small-M decoder layer (SSOUT of skinny_gemm_kernel): 16-bit or 8-bit weight rows
template <class WV>
static void resid_ss_launch(const void* X, const void* W, const float* wscale, const void* R, void* Y, float* ss_out, int M, int N, int K, int64_t ldx,
                            int64_t ldr, int64_t ldy, void* stream) {
    dim3 grid((N + 15) / 16, 1);
    hipStream_t st = (hipStream_t)stream;
    if (N <= 8192 && K % 256 == 0 && eight_wave_blocks(N))
        hipLaunchKernelGGL((skinny_gemm_kernel<1, 8, true, WV>), grid, dim3(512), 0, st, (const uint16_t*)X, (const typename WV::code_t*)W,
                           (const uint16_t*)R, (uint16_t*)Y, (float*)nullptr, M, N, K, (long long)ldx, (long long)ldr, (long long)ldy, ss_out, wscale);
    else
        hipLaunchKernelGGL((skinny_gemm_kernel<1, 4, true, WV>), grid, dim3(256), 0, st, (const uint16_t*)X, (const typename WV::code_t*)W,
                           (const uint16_t*)R, (uint16_t*)Y, (float*)nullptr, M, N, K, (long long)ldx, (long long)ldr, (long long)ldy, ss_out, wscale);
}

// Persistent blocks of the normalise-once projections: two 4-wave blocks per CU while two copies of the normalised rows fit in the
// 160 KiB of LDS; beyond that (>= 10 rows of 4096) ONE 8-wave block per CU, so that as many W bytes are in flight per CU as before
// (12 rows, gate/up: 48.6 us with one 4-wave block, 64 us with 512 blocks in two rounds - each round repeats the prologue).
static constexpr size_t NORMED_LDS_CAP = 142 * 1024;                 // + 16.5 KiB static (two partial-sum buffers of 8 waves)
struct NormedPlan { int grid; bool wide; };
static NormedPlan normed_plan(int n_cb, size_t lds_bytes) {
    const bool two = 2 * (lds_bytes + 9 * 1024) <= 160 * 1024;
    const int g = (two ? 2 : 1) * cu_count();
    return NormedPlan{n_cb < g ? n_cb : g, !two};
}
template <bool SWIGLU, class WV = Rows16>
static int normed_launch(const void* H, const float* ss, int nss, const void* ln_w, float eps, const void* W, const float* wscale, void* Y, int M,
                         int N, int K, int64_t ldh, int64_t ldy, int n_cb, void* stream) {
    const size_t lds = (size_t)M * 2 * (size_t)K;
    if (lds > NORMED_LDS_CAP || K > 8192 || nss > 512) return VDD_ERR_UNSUPPORTED;
    const NormIn ni{ss, nss, (const uint16_t*)ln_w, eps};
    const NormedPlan pl = normed_plan(n_cb, lds);
#define VDD_NORMED(NW, R)                                                                                                              \
    do {                                                                                                                               \
        static bool attr = false;                                                                                                      \
        if (!attr) { (void)hipFuncSetAttribute((const void*)skinny_normed_kernel<NW, SWIGLU, R, WV>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                               (int)NORMED_LDS_CAP); attr = true; }                                                    \
        hipLaunchKernelGGL((skinny_normed_kernel<NW, SWIGLU, R, WV>), dim3(pl.grid), dim3(NW * 64), lds, (hipStream_t)stream,          \
                           (const uint16_t*)H, (const typename WV::code_t*)W, (uint16_t*)Y, M, N, K, (long long)ldh, (long long)ldy, ni, \
                           n_cb, wscale);                                                                                              \
    } while (0)
    if (pl.wide) { if (M <= 8) VDD_NORMED(8, 8); else VDD_NORMED(8, 16); }
    else if (M <= 2) VDD_NORMED(4, 2);
    else if (M <= 4) VDD_NORMED(4, 4);
    else if (M <= 8) VDD_NORMED(4, 8);
    else VDD_NORMED(4, 16);
#undef VDD_NORMED
    return ok(hipSuccess);
}

}  // namespace VDD_ELEM_NS
}  // namespace

using namespace VDD_ELEM_NS;

extern "C" {

VDD_HIDDEN int VDD_IMPL(vdd_rmsnorm)(const void* x, const void* delta, const float* delta_slabs, int n_slabs, const void* w, void* y, void* resid_out,
                int M, int d, float eps, void* stream) {
    if (M <= 0) return VDD_OK;
    if (!x || !w || !y || d % 8 != 0 || d > 8192 || (delta && delta_slabs) || (delta_slabs && n_slabs < 1)) return VDD_ERR_INVALID_ARG;
    const float* Sl = delta_slabs; const long long ss = (long long)M * d;
    hipStream_t st = (hipStream_t)stream;
    auto X = (const uint16_t*)x; auto Dl = (const uint16_t*)delta; auto Wt = (const uint16_t*)w; auto Y = (uint16_t*)y; auto Ro = (uint16_t*)resid_out;
    const int vpt = (d / 8 + 255) / 256;
    // decode-size batches: the residual stream crosses the chip once per kernel (nontemporal); at prefill size the next kernel still
    // finds part of it in the Infinity Cache, and there the hint costs 2 % of the prefill
    const int stream_io = M <= 8192 ? 1 : 0;
    if (vpt <= 1) hipLaunchKernelGGL(rmsnorm_kernel<1>, dim3(M), dim3(256), 0, st, X, Dl, Sl, n_slabs, ss, Wt, Y, Ro, d, eps, stream_io);
    else if (vpt <= 2) hipLaunchKernelGGL(rmsnorm_kernel<2>, dim3(M), dim3(256), 0, st, X, Dl, Sl, n_slabs, ss, Wt, Y, Ro, d, eps, stream_io);
    else hipLaunchKernelGGL(rmsnorm_kernel<4>, dim3(M), dim3(256), 0, st, X, Dl, Sl, n_slabs, ss, Wt, Y, Ro, d, eps, stream_io);
    return ok(hipSuccess);
}

VDD_HIDDEN int VDD_IMPL(vdd_rope_kv_write)(const void* qkv, const int* pos, const int* cpos, const int* slot, const float* cos_sin, void* q_out, void* k_cache,
                      void* v_cache, int M, int Hq, int Hkv, int D, int64_t slot_stride, int t_max, void* stream) {
    if (M <= 0) return VDD_OK;
    if (!qkv || !pos || !cpos || !slot || !cos_sin || !q_out || !k_cache || !v_cache || D % 16 != 0) return VDD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(rope_kv_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)qkv, pos, cpos, slot, cos_sin,
                       (uint16_t*)q_out, (uint16_t*)k_cache, (uint16_t*)v_cache, Hq, Hkv, D, (long long)slot_stride, t_max, M <= 8192 ? 1 : 0);
    return ok(hipSuccess);
}

VDD_HIDDEN int VDD_IMPL(vdd_rope_kv_write_paged)(const void* qkv, const int* pos, const int* cpos, const int* slot, const float* cos_sin, void* q_out,
                            void* k_pages, void* v_pages, const int32_t* page_table, int M, int Hq, int Hkv, int D, int64_t page_stride,
                            int n_pages, int n_slots, int max_pages_per_slot, void* stream) {
    if (M <= 0) return VDD_OK;
    if (!qkv || !pos || !cpos || !slot || !cos_sin || !q_out || D % 16 != 0 ||
        !paged_args_ok(k_pages, v_pages, page_table, Hkv, D, page_stride, n_pages, n_slots, max_pages_per_slot)) return VDD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(rope_kv_paged_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)qkv, pos, cpos, slot, cos_sin,
                       (uint16_t*)q_out, (uint16_t*)k_pages, (uint16_t*)v_pages, PageTable{page_table, n_slots, max_pages_per_slot, n_pages},
                       Hq, Hkv, D, M <= 8192 ? 1 : 0);
    return ok(hipSuccess);
}

VDD_HIDDEN int VDD_IMPL(vdd_kv_pages_scatter)(const void* k_own, const void* v_own, void* k_pages, void* v_pages, const int32_t* page_table,
                         const int32_t* slots, const int32_t* n_tok, int M, int max_tok, int Hkv, int D, int64_t slot_stride, int t_max,
                         int64_t page_stride, int n_pages, int n_slots, int max_pages_per_slot, void* stream) {
    if (M <= 0 || max_tok <= 0) return VDD_OK;
    if (!k_own || !v_own || !slots || !n_tok || M > 65535 || t_max <= 0 || slot_stride < (int64_t)Hkv * t_max * D ||
        !paged_args_ok(k_pages, v_pages, page_table, Hkv, D, page_stride, n_pages, n_slots, max_pages_per_slot)) return VDD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(kv_pages_scatter_kernel, dim3(max_tok < t_max ? max_tok : t_max, M), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)k_own, (const uint16_t*)v_own, (uint16_t*)k_pages, (uint16_t*)v_pages,
                       PageTable{page_table, n_slots, max_pages_per_slot, n_pages}, slots, n_tok, Hkv, D, (long long)slot_stride, t_max, n_slots);
    return ok(hipSuccess);
}

VDD_HIDDEN int VDD_IMPL(vdd_silu_mul)(const void* gate_up, void* out, int64_t M, int F, void* stream) {
    if (M <= 0) return VDD_OK;
    if (!gate_up || !out || F % 8 != 0) return VDD_ERR_INVALID_ARG;
    if (M > 65535) {        // gridDim.y limit: launch in row slabs
        for (int m0 = 0; m0 < M; m0 += 65535) {
            const int mm = M - m0 < 65535 ? M - m0 : 65535;
            hipLaunchKernelGGL(silu_mul_kernel, dim3((F / 8 + 255) / 256, mm), dim3(256), 0, (hipStream_t)stream,
                               (const uint16_t*)gate_up + (size_t)m0 * 2 * F, (uint16_t*)out + (size_t)m0 * F, (long long)mm, F);
        }
        return ok(hipSuccess);
    }
    hipLaunchKernelGGL(silu_mul_kernel, dim3((F / 8 + 255) / 256, M), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)gate_up, (uint16_t*)out, (long long)M, F);
    return ok(hipSuccess);
}

VDD_HIDDEN int VDD_IMPL(vdd_embed)(const int64_t* ids, const void* table, void* out, int M, int d, int vocab, void* stream) {
    if (M <= 0) return VDD_OK;
    if (!ids || !table || !out || d % 8 != 0 || vocab <= 0) return VDD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(embed_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, (const long long*)ids, (const uint16_t*)table, (uint16_t*)out, d, vocab);
    return ok(hipSuccess);
}

VDD_HIDDEN int VDD_IMPL(vdd_embed_scatter)(const int32_t* ids, const int32_t* rows, const void* table, void* out, int M, int d, int vocab, void* stream) {
    if (M <= 0) return VDD_OK;
    if (!ids || !rows || !table || !out || d % 8 != 0 || vocab <= 0) return VDD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(embed_scatter_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, ids, rows, (const uint16_t*)table, (uint16_t*)out, d, vocab);
    return ok(hipSuccess);
}

VDD_HIDDEN int VDD_IMPL(vdd_skinny_gemm)(const void* X, const void* W, const void* R, void* Y, float* Y_slabs, int n_split, int M, int N, int K,
                    int64_t ldx, int64_t ldr, int64_t ldy, void* stream) {
    if (M <= 0 || N <= 0) return VDD_OK;
    if (!X || !W || (!Y && !Y_slabs) || n_split < 1 || K % (128 * n_split) != 0 || M > 64 || (ldx % 8) != 0) return VDD_ERR_INVALID_ARG;
    if (!Y_slabs && n_split != 1) return VDD_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((N + 15) / 16, n_split);
    auto x = (const uint16_t*)X; auto w = (const uint16_t*)W; auto r = (const uint16_t*)R; auto y = (uint16_t*)Y;
    if (M > 16 && n_split == 1 && Y != nullptr && K % 256 == 0 && N > 8192) {          // 17 - 64 rows, wide outputs: 32 columns per block
        wide_launch<false>(x, w, r, y, M, N, K, ldx, ldr, ldy, st);
        return ok(hipSuccess);
    }
#define VDD_SKINNY(MT, NW) hipLaunchKernelGGL((skinny_gemm_kernel<MT, NW>), grid, dim3(NW * 64), 0, st, x, w, r, y, Y_slabs, M, N, K, (long long)ldx, (long long)ldr, (long long)ldy, (float*)nullptr, (const float*)nullptr)
    // few column blocks (N = d projections): eight waves per block split K eight ways instead of fp32 slabs across blocks
    if (M <= 16 && n_split == 1 && N <= 8192 && K % 256 == 0 && eight_wave_blocks(N)) VDD_SKINNY(1, 8);
    else if (M <= 16) VDD_SKINNY(1, 4);
    else if (M <= 32) VDD_SKINNY(2, 4); else VDD_SKINNY(4, 4);
#undef VDD_SKINNY
    return ok(hipSuccess);
}

VDD_HIDDEN int VDD_IMPL(vdd_skinny_swiglu)(const void* X, const void* W_gate_up, void* act, int M, int F, int K, int64_t ldx, void* stream) {
    if (M <= 0 || F <= 0) return VDD_OK;
    if (!X || !W_gate_up || !act || M > 64 || K % 128 != 0 || (ldx % 8) != 0 || (M > 16 && K % 256 != 0)) return VDD_ERR_INVALID_ARG;
    if (M > 16)                                                             // 17 - 64 rows: 16 features (gate + up tiles) per block
        wide_launch<true>((const uint16_t*)X, (const uint16_t*)W_gate_up, nullptr, (uint16_t*)act, M, F, K, ldx, 0, (int64_t)F, (hipStream_t)stream);
    else
        hipLaunchKernelGGL(skinny_swiglu_kernel<Rows16>, dim3((F + 7) / 8), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)X,
                           (const uint16_t*)W_gate_up, (uint16_t*)act, M, F, K, (long long)ldx, (const float*)nullptr);
    return ok(hipSuccess);
}

// ---- small-M decoder-layer fusions of the RMSNorm launches (see skinny_gemm_kernel)
VDD_HIDDEN int VDD_IMPL(vdd_skinny_gemm_resid_ss)(const void* X, const void* W, const void* R, void* Y, float* ss_out, int M, int N, int K, int64_t ldx,
                             int64_t ldr, int64_t ldy, void* stream) {
    if (M <= 0 || N <= 0) return VDD_OK;
    if (!X || !W || !R || !Y || !ss_out || M > 16 || K % 128 != 0 || (ldx % 8) != 0) return VDD_ERR_INVALID_ARG;
    resid_ss_launch<Rows16>(X, W, nullptr, R, Y, ss_out, M, N, K, ldx, ldr, ldy, stream);
    return ok(hipSuccess);
}

VDD_HIDDEN int VDD_IMPL(vdd_skinny_gemm_normed)(const void* H, const float* ss, int nss, const void* ln_w, float eps, const void* W, void* Y, int M, int N,
                           int K, int64_t ldh, int64_t ldy, void* stream) {
    if (M <= 0 || N <= 0) return VDD_OK;
    if (!H || !ss || nss <= 0 || (nss % 4) != 0 || !ln_w || !W || !Y || M > 16 || K % 256 != 0 || (ldh % 8) != 0) return VDD_ERR_INVALID_ARG;
    return normed_launch<false>(H, ss, nss, ln_w, eps, W, nullptr, Y, M, N, K, ldh, ldy, (N + 15) / 16, stream);
}

VDD_HIDDEN int VDD_IMPL(vdd_skinny_swiglu_normed)(const void* H, const float* ss, int nss, const void* ln_w, float eps, const void* W_gate_up, void* act,
                             int M, int F, int K, int64_t ldh, void* stream) {
    if (M <= 0 || F <= 0) return VDD_OK;
    if (!H || !ss || nss <= 0 || (nss % 4) != 0 || !ln_w || !W_gate_up || !act || M > 16 || K % 256 != 0 || (ldh % 8) != 0) return VDD_ERR_INVALID_ARG;
    return normed_launch<true>(H, ss, nss, ln_w, eps, W_gate_up, nullptr, act, M, F, K, ldh, (int64_t)F, (F + 7) / 8, stream);
}

// ---- the same three entries on 8-bit weights (e4m3 codes + a power-of-two scale per row, RowsW8): bit for bit the 16-bit entry on the
// dequantised weight.  A shape outside M <= 16, K % 256 == 0 and the LDS cap is VDD_ERR_UNSUPPORTED: the caller runs the 16-bit twin.
VDD_HIDDEN int VDD_IMPL(vdd_skinny_gemm_resid_ss_w8)(const void* X, const void* W8, const float* w_scale, const void* R, void* Y, float* ss_out, int M,
                                int N, int K, int64_t ldx, int64_t ldr, int64_t ldy, void* stream) {
    if (M <= 0 || N <= 0) return VDD_OK;
    if (!X || !W8 || !w_scale || !R || !Y || !ss_out || (ldx % 8) != 0) return VDD_ERR_INVALID_ARG;
    if (M > 16 || K <= 0 || K % 256 != 0) return VDD_ERR_UNSUPPORTED;
    resid_ss_launch<RowsW8>(X, W8, w_scale, R, Y, ss_out, M, N, K, ldx, ldr, ldy, stream);
    return ok(hipSuccess);
}

VDD_HIDDEN int VDD_IMPL(vdd_skinny_gemm_normed_w8)(const void* H, const float* ss, int nss, const void* ln_w, float eps, const void* W8,
                              const float* w_scale, void* Y, int M, int N, int K, int64_t ldh, int64_t ldy, void* stream) {
    if (M <= 0 || N <= 0) return VDD_OK;
    if (!H || !ss || nss <= 0 || (nss % 4) != 0 || !ln_w || !W8 || !w_scale || !Y || (ldh % 8) != 0) return VDD_ERR_INVALID_ARG;
    if (M > 16 || K <= 0 || K % 256 != 0) return VDD_ERR_UNSUPPORTED;
    return normed_launch<false, RowsW8>(H, ss, nss, ln_w, eps, W8, w_scale, Y, M, N, K, ldh, ldy, (N + 15) / 16, stream);
}

VDD_HIDDEN int VDD_IMPL(vdd_skinny_swiglu_normed_w8)(const void* H, const float* ss, int nss, const void* ln_w, float eps, const void* W8_gate_up,
                                const float* w_scale, void* act, int M, int F, int K, int64_t ldh, void* stream) {
    if (M <= 0 || F <= 0) return VDD_OK;
    if (!H || !ss || nss <= 0 || (nss % 4) != 0 || !ln_w || !W8_gate_up || !w_scale || !act || (ldh % 8) != 0) return VDD_ERR_INVALID_ARG;
    if (M > 16 || K <= 0 || K % 256 != 0) return VDD_ERR_UNSUPPORTED;
    return normed_launch<true, RowsW8>(H, ss, nss, ln_w, eps, W8_gate_up, w_scale, act, M, F, K, ldh, (int64_t)F, (F + 7) / 8, stream);
}

// ---- the plain weight-streaming entries on 8-bit weight rows: every dispatch branch vdd_skinny_gemm / vdd_skinny_swiglu take for a call
// without residual and without slabs, bit for bit the 16-bit entry on w16.  M > 64 or K % 256 != 0 is VDD_ERR_UNSUPPORTED (nothing launched).
VDD_HIDDEN int VDD_IMPL(vdd_skinny_gemm_w8)(const void* X, const void* W8, const float* w_scale, void* Y, int M, int N, int K, int64_t ldx, int64_t ldy,
                       void* stream) {
    if (M <= 0 || N <= 0) return VDD_OK;
    if (!X || !W8 || !w_scale || !Y || (ldx % 8) != 0) return VDD_ERR_INVALID_ARG;
    if (M > 64 || K <= 0 || K % 256 != 0) return VDD_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((N + 15) / 16, 1);
    auto x = (const uint16_t*)X; auto w = (const uint8_t*)W8; auto y = (uint16_t*)Y;
    if (M > 16 && N > 8192) {
        wide_w8_launch<false>(x, w, w_scale, y, M, N, K, ldx, ldy, st);
        return ok(hipSuccess);
    }
#define VDD_SKINNY_W8(MT, NW) hipLaunchKernelGGL((skinny_gemm_kernel<MT, NW, false, RowsW8>), grid, dim3(NW * 64), 0, st, x, w, (const uint16_t*)nullptr, y, (float*)nullptr, M, N, K, (long long)ldx, 0ll, (long long)ldy, (float*)nullptr, w_scale)
    if (M <= 16 && N <= 8192 && eight_wave_blocks(N)) VDD_SKINNY_W8(1, 8);
    else if (M <= 16) VDD_SKINNY_W8(1, 4);
    else if (M <= 32) VDD_SKINNY_W8(2, 4); else VDD_SKINNY_W8(4, 4);
#undef VDD_SKINNY_W8
    return ok(hipSuccess);
}

VDD_HIDDEN int VDD_IMPL(vdd_skinny_swiglu_w8)(const void* X, const void* W8_gate_up, const float* w_scale, void* act, int M, int F, int K, int64_t ldx,
                         void* stream) {
    if (M <= 0 || F <= 0) return VDD_OK;
    if (!X || !W8_gate_up || !w_scale || !act || (ldx % 8) != 0) return VDD_ERR_INVALID_ARG;
    if (M > 64 || K <= 0 || K % 256 != 0) return VDD_ERR_UNSUPPORTED;
    if (M > 16)
        wide_w8_launch<true>((const uint16_t*)X, (const uint8_t*)W8_gate_up, w_scale, (uint16_t*)act, M, F, K, ldx, (int64_t)F, (hipStream_t)stream);
    else
        hipLaunchKernelGGL(skinny_swiglu_kernel<RowsW8>, dim3((F + 7) / 8), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)X,
                           (const uint8_t*)W8_gate_up, (uint16_t*)act, M, F, K, (long long)ldx, w_scale);
    return ok(hipSuccess);
}

}  // extern "C"
