// Decode attention of the branch-batched LLaVA language model for gfx950 (MI355X): one query per (row, head) over a ragged,
// prefix-shared KV cache.  Context of a row = [prefix slot: tokens 0..plen) ++ [own slot: tokens plen..len): rows that share a
// prompt prefix (same image + system prompt) point at ONE physical copy.  Compiled once per storage type (csrc/vdd_elem.h);
// accumulation fp32.  HBM-bound throughout.
//
//   vdd_decode_attention                   split-KV: decode_attn_kernel (64-key chunks -> partials) + decode_attn_combine_kernel
//   vdd_decode_attention_paged             the same over the paged own-KV pool: decode_attn_paged_kernel + combine
//   vdd_decode_attention_grouped           shared prefixes once per group on the matrix cores (decode_attn_prefix_mfma_kernel), then
//                                          the own keys: decode_attn_own_merge_kernel (<= 256 own keys) or decode_attn_kernel + combine
//   vdd_decode_attention_shared_invariant  batch-invariant mode with shared prefixes: the MFMA prefix pass with a batch-free chunk walk, then
//                                          decode_attn_mixed_kernel (per row: own chunks behind the prefix, or whole-context chunks) + combine
//   vdd_decode_attention_grouped_list      the grouped form for a work list that changes under ONE captured launch: decode_attn_prefix_mfma_kernel<.., LIST>
//                                          (item count from device memory, strided walk); own keys contiguous or through the page table
//                                          (decode_attn_own_merge_paged_kernel / decode_attn_paged_own_kernel + combine)
//   vdd_decode_attention_shared_invariant_list  the batch-invariant form on such a list (contiguous own pool)
//   vdd_decode_attention_fused             few rows: RoPE + KV-cache write + whole-context attention + merge in ONE kernel
//   vdd_decode_attention_fused_split       ... with the old keys split 2 or 4 ways across blocks (ticket merge)
//   vdd_prefix_fragments                   fragment-major copy of a prefix's K / V for the MFMA prefix pass (once per generate)
//   vdd_decode_attention_workspace_bytes, vdd_decode_attention_fused_split_workspace_bytes
//
// No projection form (form_choices_mi355x.json) chooses between kernels of this file.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vdd_llm_common.h"

namespace {
namespace VDD_ELEM_NS {

typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;
typedef __attribute__((ext_vector_type(2))) float f32x2_hw;

// One key of the online softmax for a 16-lane group: s is already reduced over the group.  The running maximum only
// moves on a small fraction of the keys, so the rescale of (l, acc) is taken lazily behind a wave-uniform test and
// the common path is 8 converts + 8 FMAs.
#define ATT_ONLINE_STEP(s, vv, m, l, acc)                                                                      \
    do {                                                                                                       \
        if (__any((s) > (m))) {                                                                                \
            const float mn_ = fmaxf((m), (s));                                                                 \
            const float corr_ = __expf((m) - mn_);                                                             \
            (l) *= corr_;                                                                                      \
            _Pragma("unroll") for (int e_ = 0; e_ < 8; ++e_) (acc)[e_] *= corr_;                                \
            (m) = mn_;                                                                                         \
        }                                                                                                      \
        const float p_ = __expf((s) - (m));                                                                    \
        (l) += p_;                                                                                             \
        (acc)[0] += p_ * lo((vv).x); (acc)[1] += p_ * hi((vv).x); (acc)[2] += p_ * lo((vv).y); (acc)[3] += p_ * hi((vv).y); \
        (acc)[4] += p_ * lo((vv).z); (acc)[5] += p_ * hi((vv).z); (acc)[6] += p_ * lo((vv).w); (acc)[7] += p_ * hi((vv).w); \
    } while (0)

// the score of one key for a 16-lane group (lane j holds dims 8j..8j+7 of q and of the key): every lane of the group gets q.k * scale
__device__ __forceinline__ float key_score(const uint4& qv, const uint4& kv, float scale) {
    float s = dot8(qv, kv);
    s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8);
    return s * scale;
}
// merge the online-softmax states of the wave's 4 lane groups (xor 16, 32): afterwards every group holds the whole wave's state
__device__ __forceinline__ void merge_lane_groups(float& m, float& l, float (&acc)[8]) {
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const float mo = __shfl_xor(m, o), lo_ = __shfl_xor(l, o);
        const float mn = fmaxf(m, mo);
        const float c0 = (m == -INFINITY) ? 0.f : __expf(m - mn), c1 = (mo == -INFINITY) ? 0.f : __expf(mo - mn);
        l = l * c0 + lo_ * c1;
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float ao = __shfl_xor(acc[e], o); acc[e] = acc[e] * c0 + ao * c1; }
        m = mn;
    }
}
// the normalised output row of a wave whose lane owns dims 2 lane, 2 lane + 1: (a0, a1) / L
__device__ __forceinline__ void store_out_pair(uint16_t* orow, int lane, float a0, float a1, float L) {
    const float inv = 1.f / L;
    reinterpret_cast<uint32_t*>(orow)[lane] = pack(a0 * inv, a1 * inv);
}

// ------------------------------------------------------------------ split-KV decode attention
// One wave per (row, head).  Lane group g = lane>>4 takes keys t = 4i + g, lane j = lane&15 the
// dims 8j..8j+7: per iteration a wave reads 4 consecutive K rows (1 KiB contiguous) and the 4
// matching V rows.  Each group runs its own online softmax; the 4 partial states merge at the
// end.
struct AttnRow { int slot, len, pslot, plen; };

// Split-KV form: blockIdx.z = key chunk of CH keys; every (row, head, chunk) wave leaves an
// un-normalised partial (acc[128], m, l) in `ws`, and decode_attn_combine merges the chunks.
// The split turns one ~650-iteration latency chain per (row, head) into <= CH/4 iterations with
// 8 x 16-B loads in flight per lane, and multiplies the number of independent waves by T/CH.
constexpr int ATT_CH = 64;
// a partial of the split-KV attention: D un-normalised output floats, then (running max, sum); records are 528 B so that every
// store of one is 16-byte aligned (520-byte records cost the prefix pass 10 us of partial-line write traffic: tools/probes/hbm_stream_probe.hip)
constexpr int ATT_PS = 128 + 4;

// Where the own keys of a row live.  `at(ar, kvh, j, Hkv)` is called once per wave and returns the wave's view: k(tt) / v(tt) = the
// address of the lane's 8 dims of own key tt (absolute index, plen <= tt < len; any tt must give a VALID address: the loop loads
// before it tests), ok(tt) = whether the key exists.
template <int D>
struct OwnContiguous {      // compact slots [n_slots, Hkv, t_max, D]: token tt at index tt - plen of slot ar.slot
    const uint16_t *kc, *vc; long long slot_stride; int t_max;
    struct View {
        const uint16_t *kb, *vb;
        __device__ __forceinline__ const uint16_t* k(int tt) const { return kb + (size_t)tt * D; }
        __device__ __forceinline__ const uint16_t* v(int tt) const { return vb + (size_t)tt * D; }
        __device__ __forceinline__ bool ok(int) const { return true; }
    };
    __device__ __forceinline__ View at(const AttnRow& ar, int kvh, int j, int) const {
        const size_t hoff = (size_t)kvh * t_max * D + j * 8;
        return View{kc + (size_t)ar.slot * slot_stride + hoff - (size_t)ar.plen * D, vc + (size_t)ar.slot * slot_stride + hoff - (size_t)ar.plen * D};
    }
};
template <int D>
struct OwnPaged {           // page pools [n_pages, Hkv, KV_PAGE, D] behind the page table: ONE table entry per key (a table row is a few dozen
    const uint16_t *kp, *vp; PageTable pt;      // ints shared by all waves of the row: it stays in cache).  A key without a page is read
    struct View {                               // from page 0 and left out of the softmax.
        const uint16_t *kp, *vp; PageTable pt; int slot, plen; size_t hoff; long long page_stride;
        __device__ __forceinline__ size_t off(int tt) const {
            const int i = tt > plen ? tt - plen : 0, pg = page_of(pt, slot, i);
            return (size_t)(pg < 0 ? 0 : pg) * page_stride + hoff + (size_t)(i & (KV_PAGE - 1)) * D;
        }
        __device__ __forceinline__ const uint16_t* k(int tt) const { return kp + off(tt); }
        __device__ __forceinline__ const uint16_t* v(int tt) const { return vp + off(tt); }
        __device__ __forceinline__ bool ok(int tt) const { return tt < plen || page_of(pt, slot, tt - plen) >= 0; }
    };
    __device__ __forceinline__ View at(const AttnRow& ar, int kvh, int j, int Hkv) const {
        return View{kp, vp, pt, ar.slot, ar.plen, (size_t)kvh * KV_PAGE * D + j * 8, (long long)Hkv * KV_PAGE * D};
    }
};

// The work of one (row, head, chunk) wave - ONE body for the contiguous and the paged kernel, so that both walk the same 64-key
// chunks with the same lane-group-to-key map and the same online-softmax order: equal K / V give equal bits.
template <int D, class Own>   // head dim 128
__device__ __forceinline__ void decode_attn_chunk(const uint16_t* __restrict__ q, const Own pool, const uint16_t* __restrict__ kpre,
                                                  const uint16_t* __restrict__ vpre, const AttnRow* __restrict__ rows, float* __restrict__ ws,
                                                  int H, int Hkv, long long pre_stride, int pre_tmax, float scale, int nchunk,
                                                  int own_only, int chunk_base) {
    static_assert(D == 128, "lane map assumes 16 lanes x 8 dims");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int head = blockIdx.x * 4 + wave, row = blockIdx.y, chunk = blockIdx.z;
    if (head >= H) return;
    const int g = lane >> 4, j = lane & 15;
    const AttnRow ar = rows[row];
    float* wsp = ws + (((size_t)row * H + head) * nchunk + chunk_base + chunk) * ATT_PS;
    // own_only: the shared prefix [0, plen) is handled by the grouped MFMA kernel; this one starts at plen
    const int k0 = (own_only ? ar.plen : 0) + chunk * ATT_CH, k1 = min(ar.len, k0 + ATT_CH);
    if (k0 >= ar.len) {                                   // empty chunk: neutral partial
        if (lane == 0) { wsp[D] = -INFINITY; wsp[D + 1] = 0.f; }
        return;
    }
    const int kvh = head / (H / Hkv);
    const uint4 qv = *reinterpret_cast<const uint4*>(q + ((size_t)row * H + head) * D + j * 8);
    // own pool stores token t at index t - plen (compact slots or pages); the prefix pool at index t
    const size_t poff = (size_t)kvh * pre_tmax * D + j * 8;
    const auto own = pool.at(ar, kvh, j, Hkv);
    const uint16_t* k_pre = kpre + (size_t)ar.pslot * pre_stride + poff;
    const uint16_t* v_pre = vpre + (size_t)ar.pslot * pre_stride + poff;
    float m = -INFINITY, l = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    constexpr int U = 4;
    for (int t0 = k0 + g; t0 < k1; t0 += 4 * U) {
        uint4 kv[U], vv[U];
        bool there[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 + 4 * u;
            const int tt = t < k1 ? t : k1 - 1;
            const bool pre = tt < ar.plen;
            kv[u] = ld_stream(pre ? k_pre + (size_t)tt * D : own.k(tt));        // each K / V row is read by one wave of the launch
            vv[u] = ld_stream(pre ? v_pre + (size_t)tt * D : own.v(tt));
            there[u] = t < k1 && own.ok(tt);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float s = key_score(qv, kv[u], scale);
            if (there[u]) ATT_ONLINE_STEP(s, vv[u], m, l, acc);
        }
    }
    merge_lane_groups(m, l, acc);
    if (g == 0) {
        *reinterpret_cast<float4*>(wsp + j * 8) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        *reinterpret_cast<float4*>(wsp + j * 8 + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
        if (j == 0) { wsp[D] = m; wsp[D + 1] = l; }
    }
}

template <int D>
__global__ void __launch_bounds__(256) decode_attn_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ kc,
                                                          const uint16_t* __restrict__ vc, const uint16_t* __restrict__ kpre,
                                                          const uint16_t* __restrict__ vpre, const AttnRow* __restrict__ rows,
                                                          float* __restrict__ ws, int H, int Hkv, long long slot_stride,
                                                          int t_max, long long pre_stride, int pre_tmax, float scale, int nchunk,
                                                          int own_only, int chunk_base) {
    decode_attn_chunk<D>(q, OwnContiguous<D>{kc, vc, slot_stride, t_max}, kpre, vpre, rows, ws, H, Hkv, pre_stride, pre_tmax, scale, nchunk,
                         own_only, chunk_base);
}

template <int D>
__global__ void __launch_bounds__(256) decode_attn_paged_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k_pages,
                                                                const uint16_t* __restrict__ v_pages, PageTable pt,
                                                                const uint16_t* __restrict__ kpre, const uint16_t* __restrict__ vpre,
                                                                const AttnRow* __restrict__ rows, float* __restrict__ ws, int H, int Hkv,
                                                                long long pre_stride, int pre_tmax, float scale, int nchunk) {
    decode_attn_chunk<D>(q, OwnPaged<D>{k_pages, v_pages, pt}, kpre, vpre, rows, ws, H, Hkv, pre_stride, pre_tmax, scale, nchunk, 0, 0);
}

// The own chunks of the grouped form over the paged pool (vdd_decode_attention_grouped_list with a page table, own ranges above 256
// keys): decode_attn_kernel's own_only walk behind the `npre` prefix records, keys through the page table.
template <int D>
__global__ void __launch_bounds__(256) decode_attn_paged_own_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k_pages,
                                                                    const uint16_t* __restrict__ v_pages, PageTable pt,
                                                                    const uint16_t* __restrict__ kpre, const uint16_t* __restrict__ vpre,
                                                                    const AttnRow* __restrict__ rows, float* __restrict__ ws, int H, int Hkv,
                                                                    long long pre_stride, int pre_tmax, float scale, int nchunk, int npre) {
    decode_attn_chunk<D>(q, OwnPaged<D>{k_pages, v_pages, pt}, kpre, vpre, rows, ws, H, Hkv, pre_stride, pre_tmax, scale, nchunk, 1, npre);
}

// Grouped mode, short own ranges (a question's own prompt tokens + what it generated so far: <= 256 keys): ONE wave per
// (row, head) walks the whole own range [plen, len), then folds in the row's prefix partials left by the MFMA prefix pass
// and writes the normalised bf16 output - no own partials, no separate combine launch.
template <int D>
__global__ void __launch_bounds__(256) decode_attn_own_merge_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ kc,
                                                                    const uint16_t* __restrict__ vc, const AttnRow* __restrict__ rows,
                                                                    const float* __restrict__ ws, uint16_t* __restrict__ out, int H, int Hkv,
                                                                    long long slot_stride, int t_max, float scale, int nchunk, int npre,
                                                                    int pre_keys) {
    static_assert(D == 128, "lane map assumes 16 lanes x 8 dims");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int head = blockIdx.x * 4 + wave, row = blockIdx.y;
    if (head >= H) return;
    const int g = lane >> 4, j = lane & 15;
    const AttnRow ar = rows[row];
    const int kvh = head / (H / Hkv);
    const uint4 qv = *reinterpret_cast<const uint4*>(q + ((size_t)row * H + head) * D + j * 8);
    const size_t hoff = (size_t)kvh * t_max * D + j * 8;
    const uint16_t* k_own = kc + (size_t)ar.slot * slot_stride + hoff;       // compact slot: own token i at index i
    const uint16_t* v_own = vc + (size_t)ar.slot * slot_stride + hoff;
    const int n_own = ar.len - ar.plen;
    float m = -INFINITY, l = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    constexpr int U = 8;
    for (int t0 = g; t0 < n_own; t0 += 4 * U) {
        uint4 kv[U], vv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 + 4 * u;
            const int tt = t < n_own ? t : n_own - 1;
            kv[u] = ld_stream(k_own + (size_t)tt * D);
            vv[u] = ld_stream(v_own + (size_t)tt * D);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float s = key_score(qv, kv[u], scale);
            if (t0 + 4 * u < n_own) ATT_ONLINE_STEP(s, vv[u], m, l, acc);
        }
    }
    merge_lane_groups(m, l, acc);
    // fold in the prefix partials (every lane of a 16-lane group reads its 8 dims; group 0 stores)
    const int used_pre = npre > 0 ? (ar.plen + pre_keys - 1) / pre_keys : 0;
    const float* base = ws + ((size_t)row * H + head) * nchunk * ATT_PS;
    for (int c = 0; c < used_pre; ++c) {
        const float* pp = base + (size_t)c * ATT_PS;
        const float mo = pp[D], lo_ = pp[D + 1];
        const float mn = fmaxf(m, mo);
        const float c0 = (m == -INFINITY) ? 0.f : __expf(m - mn), c1 = (mo == -INFINITY) ? 0.f : __expf(mo - mn);
        const float4 a0 = *reinterpret_cast<const float4*>(pp + j * 8), a1 = *reinterpret_cast<const float4*>(pp + j * 8 + 4);
        l = l * c0 + lo_ * c1;
        acc[0] = acc[0] * c0 + a0.x * c1; acc[1] = acc[1] * c0 + a0.y * c1; acc[2] = acc[2] * c0 + a0.z * c1; acc[3] = acc[3] * c0 + a0.w * c1;
        acc[4] = acc[4] * c0 + a1.x * c1; acc[5] = acc[5] * c0 + a1.y * c1; acc[6] = acc[6] * c0 + a1.z * c1; acc[7] = acc[7] * c0 + a1.w * c1;
        m = mn;
    }
    if (g == 0) {
        const float inv = 1.f / l;
        uint4 o4;
        o4.x = pack(acc[0] * inv, acc[1] * inv); o4.y = pack(acc[2] * inv, acc[3] * inv);
        o4.z = pack(acc[4] * inv, acc[5] * inv); o4.w = pack(acc[6] * inv, acc[7] * inv);
        *reinterpret_cast<uint4*>(out + ((size_t)row * H + head) * D + j * 8) = o4;
    }
}

// decode_attn_own_merge_kernel with the own keys read through the page table (vdd_decode_attention_grouped_list with a page table):
// the same lane-group-to-key map (group g takes own keys 4 i + g, 8 in flight), the same online-softmax order and the same fold of the
// prefix partials, so equal K / V give equal bits.  A key without a page is read from page 0 and left out of the softmax.
template <int D>
__global__ void __launch_bounds__(256) decode_attn_own_merge_paged_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k_pages,
                                                                          const uint16_t* __restrict__ v_pages, PageTable pt,
                                                                          const AttnRow* __restrict__ rows, const float* __restrict__ ws,
                                                                          uint16_t* __restrict__ out, int H, int Hkv, float scale, int nchunk,
                                                                          int npre, int pre_keys) {
    static_assert(D == 128, "lane map assumes 16 lanes x 8 dims");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int head = blockIdx.x * 4 + wave, row = blockIdx.y;
    if (head >= H) return;
    const int g = lane >> 4, j = lane & 15;
    const AttnRow ar = rows[row];
    const int kvh = head / (H / Hkv);
    const uint4 qv = *reinterpret_cast<const uint4*>(q + ((size_t)row * H + head) * D + j * 8);
    const auto own = OwnPaged<D>{k_pages, v_pages, pt}.at(ar, kvh, j, Hkv);      // k(tt) / v(tt) take the absolute key index plen + i
    const int n_own = ar.len - ar.plen;
    float m = -INFINITY, l = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    constexpr int U = 8;
    for (int t0 = g; t0 < n_own; t0 += 4 * U) {
        uint4 kv[U], vv[U];
        bool there[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 + 4 * u;
            const int tt = ar.plen + (t < n_own ? t : n_own - 1);
            kv[u] = ld_stream(own.k(tt));
            vv[u] = ld_stream(own.v(tt));
            there[u] = t < n_own && own.ok(tt);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float s = key_score(qv, kv[u], scale);
            if (there[u]) ATT_ONLINE_STEP(s, vv[u], m, l, acc);
        }
    }
    merge_lane_groups(m, l, acc);
    const int used_pre = npre > 0 ? (ar.plen + pre_keys - 1) / pre_keys : 0;
    const float* base = ws + ((size_t)row * H + head) * nchunk * ATT_PS;
    for (int c = 0; c < used_pre; ++c) {
        const float* pp = base + (size_t)c * ATT_PS;
        const float mo = pp[D], lo_ = pp[D + 1];
        const float mn = fmaxf(m, mo);
        const float c0 = (m == -INFINITY) ? 0.f : __expf(m - mn), c1 = (mo == -INFINITY) ? 0.f : __expf(mo - mn);
        const float4 a0 = *reinterpret_cast<const float4*>(pp + j * 8), a1 = *reinterpret_cast<const float4*>(pp + j * 8 + 4);
        l = l * c0 + lo_ * c1;
        acc[0] = acc[0] * c0 + a0.x * c1; acc[1] = acc[1] * c0 + a0.y * c1; acc[2] = acc[2] * c0 + a0.z * c1; acc[3] = acc[3] * c0 + a0.w * c1;
        acc[4] = acc[4] * c0 + a1.x * c1; acc[5] = acc[5] * c0 + a1.y * c1; acc[6] = acc[6] * c0 + a1.z * c1; acc[7] = acc[7] * c0 + a1.w * c1;
        m = mn;
    }
    if (g == 0) {
        const float inv = 1.f / l;
        uint4 o4;
        o4.x = pack(acc[0] * inv, acc[1] * inv); o4.y = pack(acc[2] * inv, acc[3] * inv);
        o4.z = pack(acc[4] * inv, acc[5] * inv); o4.w = pack(acc[6] * inv, acc[7] * inv);
        *reinterpret_cast<uint4*>(out + ((size_t)row * H + head) * D + j * 8) = o4;
    }
}

// one wave per (row, head): lane owns dims 2*lane, 2*lane+1.  Chunk space: [0, npre) prefix chunks (grouped
// kernel; only when grouped), then own/whole-context chunks.
template <int D>
__global__ void __launch_bounds__(256) decode_attn_combine_kernel(const float* __restrict__ ws, const AttnRow* __restrict__ rows,
                                                                  uint16_t* __restrict__ out, int H, int nchunk, int npre,
                                                                  int pre_keys) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int head = blockIdx.x * 4 + wave, row = blockIdx.y;
    if (head >= H) return;
    const AttnRow ar = rows[row];
    const int used_pre = npre > 0 ? (ar.plen + pre_keys - 1) / pre_keys : 0;
    const int own_len = npre > 0 ? ar.len - ar.plen : ar.len;
    const int used_own = min(nchunk - npre, (own_len + ATT_CH - 1) / ATT_CH);
    const float* base = ws + ((size_t)row * H + head) * nchunk * ATT_PS;
    float M = -INFINITY;
    for (int c = 0; c < used_pre; ++c) M = fmaxf(M, base[c * ATT_PS + D]);
    for (int c = 0; c < used_own; ++c) M = fmaxf(M, base[(npre + c) * ATT_PS + D]);
    float L = 0.f, a0 = 0.f, a1 = 0.f;
    auto add = [&](int c) {
        const float* p = base + c * ATT_PS;
        const float w = __expf(p[D] - M);
        L += w * p[D + 1];
        const float2 v = *reinterpret_cast<const float2*>(p + 2 * lane);
        a0 += w * v.x; a1 += w * v.y;
    };
    for (int c = 0; c < used_pre; ++c) add(c);
    for (int c = 0; c < used_own; ++c) add(npre + c);
    store_out_pair(out + ((size_t)row * H + head) * D, lane, a0, a1, L);
}

// ------------------------------------------------------------------ batch-invariant mode with shared prefixes
// vdd_decode_attention_shared_invariant: what a (row, head) computes is a function of its q, its keys in key order, its len and its
// prefix length alone.  mode[row] = 1 (shared: the prefix partials come from the MFMA pass, whose chunk walk knows only head, item and
// plen; the own keys are cut at plen + 64 c) or 0 (per row: the whole context cut at 64 c, prefix keys from the row-major pool - the
// arithmetic of decode_attn_kernel, bit for bit).  Records of a row: shared = [0, npre) prefix items, then own chunks; per row = chunks from 0.
template <int D>
__global__ void __launch_bounds__(256) decode_attn_mixed_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ kc,
                                                                const uint16_t* __restrict__ vc, const uint16_t* __restrict__ kpre,
                                                                const uint16_t* __restrict__ vpre, const AttnRow* __restrict__ rows,
                                                                const int* __restrict__ mode, float* __restrict__ ws, int H, int Hkv,
                                                                long long slot_stride, int t_max, long long pre_stride, int pre_tmax,
                                                                float scale, int nchunk, int npre, int nown, int nrow) {
    const int shared = mode[blockIdx.y] != 0;
    if ((int)blockIdx.z >= (shared ? nown : nrow)) return;        // records past the row's kind would lie outside its nchunk
    decode_attn_chunk<D>(q, OwnContiguous<D>{kc, vc, slot_stride, t_max}, kpre, vpre, rows, ws, H, Hkv, pre_stride, pre_tmax, scale, nchunk,
                         shared, shared ? npre : 0);
}

// decode_attn_combine_kernel with the row's kind from `mode`: prefix items ascending, then own chunks ascending; a per-row row has no
// prefix items and its chunks start at record 0 (the same sums in the same order as the combine of vdd_decode_attention)
template <int D>
__global__ void __launch_bounds__(256) decode_attn_combine_mixed_kernel(const float* __restrict__ ws, const AttnRow* __restrict__ rows,
                                                                        const int* __restrict__ mode, uint16_t* __restrict__ out, int H,
                                                                        int nchunk, int npre, int pre_keys) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int head = blockIdx.x * 4 + wave, row = blockIdx.y;
    if (head >= H) return;
    const AttnRow ar = rows[row];
    const bool shared = mode[row] != 0;
    const int used_pre = shared ? (ar.plen + pre_keys - 1) / pre_keys : 0;
    const int own_base = shared ? npre : 0;
    const int own_len = shared ? ar.len - ar.plen : ar.len;
    const int used_own = min(nchunk - own_base, (own_len + ATT_CH - 1) / ATT_CH);
    const float* base = ws + ((size_t)row * H + head) * nchunk * ATT_PS;
    float M = -INFINITY;
    for (int c = 0; c < used_pre; ++c) M = fmaxf(M, base[c * ATT_PS + D]);
    for (int c = 0; c < used_own; ++c) M = fmaxf(M, base[(own_base + c) * ATT_PS + D]);
    float L = 0.f, a0 = 0.f, a1 = 0.f;
    auto add = [&](int c) {
        const float* p = base + c * ATT_PS;
        const float w = __expf(p[D] - M);
        L += w * p[D + 1];
        const float2 v = *reinterpret_cast<const float2*>(p + 2 * lane);
        a0 += w * v.x; a1 += w * v.y;
    };
    for (int c = 0; c < used_pre; ++c) add(c);
    for (int c = 0; c < used_own; ++c) add(own_base + c);
    store_out_pair(out + ((size_t)row * H + head) * D, lane, a0, a1, L);
}

// ------------------------------------------------------------------ small-M fused decode attention
// For a handful of rows (the reference's own operating point: ONE question = 2-3 branch rows) the step is a chain of
// latency-bound launches, so RoPE, the KV-cache write, the whole-context attention and the merge run as ONE kernel:
// block = (head, row), NW waves; key t belongs to 16-lane group (t mod 4 NW); the new token's K/V never round-trip
// through the cache (they are rotated in registers, written once per KV head, and attended from registers).
// KSPLIT > 1 (one or two questions in flight: H x M blocks would leave most CUs idle and each block three dependent fetch rounds
// deep): blockIdx.z takes the z-th slice of the old keys, leaves an un-normalised partial (128 sums, max, weight) in `ws` with
// write-through stores and draws a ticket from the (row, head) counter; the block that draws the last ticket merges the KSPLIT
// partials in slice order (deterministic) and writes the output row.  Same hand-off as the GEMM's stream-K fix-up: write-through
// (sc1) stores + s_waitcnt before a relaxed agent-scope atomic, agent-scope (sc1) loads behind it, no fences; the counter is left
// at zero for the next launch.
constexpr int ATT_FS = 128 + 4;          // floats per partial of the split form: 128 sums, max, weight, 2 pad (16-byte rows)
template <int D, int NW, int KSPLIT>
__global__ void __launch_bounds__(NW * 64) decode_attn_fused_kernel(const uint16_t* __restrict__ qkv, const int* __restrict__ pos,
                                                                    const int* __restrict__ cpos, const int* __restrict__ slot,
                                                                    const float* __restrict__ cs_table, uint16_t* __restrict__ kc,
                                                                    uint16_t* __restrict__ vc, const uint16_t* __restrict__ kpre,
                                                                    const uint16_t* __restrict__ vpre, const AttnRow* __restrict__ rows,
                                                                    uint16_t* __restrict__ out, int H, int Hkv, long long slot_stride,
                                                                    int t_max, long long pre_stride, int pre_tmax, float scale,
                                                                    float* __restrict__ ws, int* __restrict__ tickets) {
    static_assert(D == 128, "lane map assumes 16 lanes x 8 dims");
    __shared__ float part[NW][D + 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
    const int head = blockIdx.x, row = blockIdx.y, zs = KSPLIT > 1 ? (int)blockIdx.z : 0;
    const AttnRow ar = rows[row];
    const int p = pos[row], cp = cpos[row];
    const int kvh = head / (H / Hkv);
    const uint16_t* src = qkv + (size_t)row * (size_t)((H + 2 * Hkv) * D);
    // context pointers and the FIRST batch of K/V loads go out before the RoPE arithmetic (they do not depend on q)
    const size_t hoff = (size_t)kvh * t_max * D + j * 8, poff = (size_t)kvh * pre_tmax * D + j * 8;
    const uint16_t* k_own = kc + (size_t)ar.slot * slot_stride + hoff - (size_t)ar.plen * D;
    const uint16_t* v_own = vc + (size_t)ar.slot * slot_stride + hoff - (size_t)ar.plen * D;
    const uint16_t* k_pre = kpre + (size_t)ar.pslot * pre_stride + poff;
    const uint16_t* v_pre = vpre + (size_t)ar.pslot * pre_stride + poff;
    constexpr int U = 4, STEP = NW * 4;
    const int n_all = ar.len - 1;                       // keys already in the cache; the new token is attended from registers
    // this block's slice [k_lo, n_old) of them (whole STEP-key rounds per slice); the last slice also takes the new token
    const int per = KSPLIT > 1 ? ((n_all + KSPLIT * STEP - 1) / (KSPLIT * STEP)) * STEP : 0;
    const int k_lo = KSPLIT > 1 ? min(zs * per, n_all) : 0;
    const int n_old = KSPLIT > 1 ? min(k_lo + per, n_all) : n_all;
    const bool last_slice = zs == KSPLIT - 1;
    const int kl = k_lo + wave * 4 + g;
    uint4 kn_[U], vn_[U];
    auto fetch = [&](int t0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 + STEP * u;
            const int tt = t < n_old ? t : n_old - 1;
            const bool pre = tt < ar.plen;
            kn_[u] = *reinterpret_cast<const uint4*>((pre ? k_pre : k_own) + (size_t)tt * D);
            vn_[u] = *reinterpret_cast<const uint4*>((pre ? v_pre : v_own) + (size_t)tt * D);
        }
    };
    if (kl < n_old) fetch(kl);
    // rotate_half RoPE: lane j < 8 holds dims 8j.. (first half), lane j + 8 the partner dims; same rounding as rope_kv_kernel
    const float* cs = cs_table + ((size_t)p * (D / 2) + (j & 7) * 8) * 2;
    const float4 c0 = *reinterpret_cast<const float4*>(cs), c1 = *reinterpret_cast<const float4*>(cs + 4),
                 c2 = *reinterpret_cast<const float4*>(cs + 8), c3 = *reinterpret_cast<const float4*>(cs + 12);
    const float sign = j < 8 ? -1.f : 1.f;
    auto rope = [&](const uint16_t* hsrc) {
        const uint4 own = *reinterpret_cast<const uint4*>(hsrc + j * 8);
        uint4 oth;
        oth.x = __shfl_xor(own.x, 8); oth.y = __shfl_xor(own.y, 8); oth.z = __shfl_xor(own.z, 8); oth.w = __shfl_xor(own.w, 8);
        auto r2 = [&](uint32_t a, uint32_t b, float cA, float sA, float cB, float sB) {
            return pack(lo(a) * cA + (sign * lo(b)) * sA, hi(a) * cB + (sign * hi(b)) * sB);
        };
        uint4 r;
        r.x = r2(own.x, oth.x, c0.x, c0.y, c0.z, c0.w); r.y = r2(own.y, oth.y, c1.x, c1.y, c1.z, c1.w);
        r.z = r2(own.z, oth.z, c2.x, c2.y, c2.z, c2.w); r.w = r2(own.w, oth.w, c3.x, c3.y, c3.z, c3.w);
        return r;
    };
    const uint4 qv = rope(src + (size_t)head * D);
    const uint4 kn = rope(src + (size_t)(H + kvh) * D);
    const uint4 vn = *reinterpret_cast<const uint4*>(src + (size_t)(H + Hkv + kvh) * D + j * 8);
    if (last_slice && wave == 0 && g == 0 && head % (H / Hkv) == 0) {      // one writer per KV head
        const size_t o = (size_t)slot[row] * slot_stride + ((size_t)kvh * t_max + cp) * D + j * 8;
        *reinterpret_cast<uint4*>(kc + o) = kn;
        *reinterpret_cast<uint4*>(vc + o) = vn;
    }
    float m = -INFINITY, l = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int t0 = kl; t0 < n_old; t0 += STEP * U) {
        uint4 kv[U], vv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { kv[u] = kn_[u]; vv[u] = vn_[u]; }
        if (t0 + STEP * U < n_old) fetch(t0 + STEP * U);      // next batch in flight under this batch's arithmetic
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float sc = key_score(qv, kv[u], scale);
            if (t0 + STEP * u < n_old) ATT_ONLINE_STEP(sc, vv[u], m, l, acc);
        }
    }
    {   // the new token, from registers (last wave's last group is the least loaded)
        const float sc = key_score(qv, kn, scale);
        if (last_slice && wave == NW - 1 && g == 3) ATT_ONLINE_STEP(sc, vn, m, l, acc);
    }
    merge_lane_groups(m, l, acc);
    if (g == 0) {
        *reinterpret_cast<float4*>(&part[wave][j * 8]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        *reinterpret_cast<float4*>(&part[wave][j * 8 + 4]) = make_float4(acc[4], acc[5], acc[6], acc[7]);
        if (j == 0) { part[wave][D] = m; part[wave][D + 1] = l; }
    }
    __syncthreads();
    if (wave == 0) {
        float Mx = -INFINITY;
#pragma unroll
        for (int w = 0; w < NW; ++w) Mx = fmaxf(Mx, part[w][D]);
        float L = 0.f, a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float wgt = part[w][D] == -INFINITY ? 0.f : __expf(part[w][D] - Mx);       // empty waves (and a whole empty slice)
            L += wgt * part[w][D + 1];
            a0 += wgt * part[w][2 * lane]; a1 += wgt * part[w][2 * lane + 1];
        }
        if constexpr (KSPLIT == 1) {
            store_out_pair(out + ((size_t)row * H + head) * D, lane, a0, a1, L);
        } else {
            const size_t rh = (size_t)row * H + head;
            float* mine = ws + (rh * KSPLIT + zs) * ATT_FS;
            const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc((void*)mine, 0, ATT_FS * 4, 0x00020000);
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_t, f32x2_hw{a0, a1}), rp, lane * 8, 0, 16);
            if (lane == 0) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_t, f32x2_hw{Mx, L}), rp, D * 4, 0, 16);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            int ticket = 0;
            if (lane == 0) ticket = __hip_atomic_fetch_add(tickets + rh, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ticket = __builtin_amdgcn_readfirstlane(ticket);
            if (ticket == KSPLIT - 1) {                  // every other slice has published: merge in slice order
                if (lane == 0) __hip_atomic_store(tickets + rh, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void*)(ws + rh * KSPLIT * ATT_FS), 0, KSPLIT * ATT_FS * 4, 0x00020000);
                f32x2_hw av[KSPLIT], ml[KSPLIT];
#pragma unroll
                for (int k = 0; k < KSPLIT; ++k) {
                    av[k] = __builtin_bit_cast(f32x2_hw, __builtin_amdgcn_raw_buffer_load_b64(rq, (k * ATT_FS) * 4 + lane * 8, 0, 16));
                    ml[k] = __builtin_bit_cast(f32x2_hw, __builtin_amdgcn_raw_buffer_load_b64(rq, (k * ATT_FS + D) * 4, 0, 16));
                }
                float Mg = -INFINITY;
#pragma unroll
                for (int k = 0; k < KSPLIT; ++k) Mg = fmaxf(Mg, ml[k][0]);
                float Lg = 0.f, b0 = 0.f, b1 = 0.f;
#pragma unroll
                for (int k = 0; k < KSPLIT; ++k) {
                    const float wgt = ml[k][0] == -INFINITY ? 0.f : __expf(ml[k][0] - Mg);     // an empty slice weighs nothing
                    Lg += wgt * ml[k][1]; b0 += wgt * av[k][0]; b1 += wgt * av[k][1];
                }
                store_out_pair(out + rh * D, lane, b0, b1, Lg);
            }
        }
    }
}

// ------------------------------------------------------------------ prefix-grouped decode attention
// Rows that share a prompt prefix (the 6 POPE questions of one image; ALL image-free branch rows) form a group: each
// prefix K/V byte leaves HBM/L2 once per group instead of once per row.
struct GroupDesc { int row_off, n_rows, pslot, plen; };

// ------------------------------------------------------------------ prefix pass on the matrix cores
// K and V of a shared prefix are static during decoding, so a second copy is kept in FRAGMENT-MAJOR order, built once per
// generate by prefix_fragments_kernel: per (slot, kv head) and 64-key chunk one 32-KiB block = 16 K fragments + 16 V^T
// fragments, each the 1-KiB lane-linear image of one MFMA operand (lane l at byte 16 l).  Every fragment load of the pass is
// then one contiguous KiB (8 whole 128-byte lines) instead of 16 half-lines (K rows) or 4 x 256 B (a key-blocked V^T), both
// contractions take their operands straight from HBM, and the pass needs no LDS and no barrier:
//   S^T = K Q^T   A = K fragment (t, ks): lane (i, g) = 16 B of K[key_t(i)][32 ks + 8 g ..], B = Q fragment (lane (query, g))
//                 C layout: column = query, row i = 4 g + r.  The key assigned to MFMA row i is chosen as
//                 key_a(i) = k0 + 8 (i/4) + i%4 for tile a and key_b(i) = key_a(i) + 4 for tile b, so that the 8
//                 probabilities a lane holds after the softmax are the 8 CONSECUTIVE keys k0 + 8 g .. + 7:
//   O = P V       A = P fragment = those 8 registers as they are (no re-layout), B = V^T fragment (kk, nt): lane (j, g) =
//                 V[k0 + 32 kk + 8 g .. + 7][8 j + nt]: column j of output tile nt is head dim 8 j + nt, so a lane ends up with
//                 8 CONSECUTIVE dims of its 4 query rows and a partial row leaves as 16 lanes x 32 B = one contiguous 512 B.
// One wave = one (16-row slice of a group, head, item of 64-key chunks): 16 + 16 MFMAs per chunk, online softmax across the
// chunks, un-normalised partial to the workspace (merged by the own pass / decode_attn_combine_kernel).
constexpr int FRAG_CHUNK_ELEMS = 2 * ATT_CH * 128;      // bf16 elements of one chunk's block (K then V^T)
__global__ void __launch_bounds__(256) prefix_fragments_kernel(const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
                                                               uint16_t* __restrict__ frag, int t_max, const int* __restrict__ plen_of_slot) {
    // grid: (t_max / 64, n_kv_heads, n_slots); block 256: one 64-key chunk, D = 128
    constexpr int D = 128;
    const int chunk = blockIdx.x, head = blockIdx.y, slot = blockIdx.z, plen = plen_of_slot[slot], k0 = chunk * ATT_CH;
    if (k0 >= plen) return;
    const size_t base = ((size_t)slot * gridDim.y + head) * (size_t)t_max * D;
    uint16_t* out = frag + 2 * base + (size_t)chunk * FRAG_CHUNK_ELEMS;
    const uint4 zero = make_uint4(0, 0, 0, 0);          // keys past the prefix: they meet p = 0 in the MFMA and must be finite
    __shared__ uint16_t tile[ATT_CH][D + 8];
    for (int p = threadIdx.x; p < ATT_CH * D / 8; p += 256) {
        const int key = p / (D / 8), c = p % (D / 8);
        *reinterpret_cast<uint4*>(&tile[key][c * 8]) = k0 + key < plen ? *reinterpret_cast<const uint4*>(v + base + (size_t)(k0 + key) * D + c * 8) : zero;
    }
    for (int p = threadIdx.x; p < 1024; p += 256) {     // K fragments: 16-byte pieces of K rows, re-ordered
        const int t = p >> 8, ks = (p >> 6) & 3, lane = p & 63, ln = lane & 15, g = lane >> 4;
        const int key = k0 + (t >> 1) * 32 + (ln >> 2) * 8 + (t & 1) * 4 + (ln & 3);
        st_stream(out + (size_t)p * 8, key < plen ? *reinterpret_cast<const uint4*>(k + base + (size_t)key * D + ks * 32 + g * 8) : zero);      // read again only by the decode steps
    }
    __syncthreads();
    for (int p = threadIdx.x; p < 1024; p += 256) {     // V^T fragments: 8 keys of one dim per lane
        const int kk = p >> 9, nt = (p >> 6) & 7, lane = p & 63, ln = lane & 15, g = lane >> 4;
        uint16_t e[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) e[i] = tile[kk * 32 + g * 8 + i][ln * 8 + nt];
        uint4 o;
        o.x = e[0] | ((uint32_t)e[1] << 16); o.y = e[2] | ((uint32_t)e[3] << 16); o.z = e[4] | ((uint32_t)e[5] << 16); o.w = e[6] | ((uint32_t)e[7] << 16);
        st_stream(out + ATT_CH * D + (size_t)p * 8, o);
    }
}

// waves-per-SIMD hint 4: left alone the compiler hoists all 16 K (then V) fragment loads of a chunk and lands at 140
// registers = 3 waves per SIMD; capped at 128 the pass is 10 % faster (tools/attn_probe.py: 314 -> 274 us per layer).
// INVARIANT (vdd_decode_attention_shared_invariant): the chunk walk of an item may know the head, the item's index inside the prefix and
// plen, never the group, the slice or the slot - a row's partial must not change with its neighbours.
// LIST (vdd_decode_attention_grouped_list / _shared_invariant_list): a work list that changes between replays of ONE captured launch
// (engine.generate_list(group_images=True): group membership moves with every admission, release and preemption).  The item count is
// read from device memory (clamped to the capacity of `items`) and the blocks walk the list with a stride of gridDim.y, which the host
// sizes from the list's capacity and the chip, never from the live count.  Which block serves an item is not part of its arithmetic:
// the same chunk walk and rotation, the same partial record.
template <int D, bool INVARIANT = false, bool LIST = false>
__global__ void __launch_bounds__(256, 2) decode_attn_prefix_mfma_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ frag,
                                                                      const GroupDesc* __restrict__ groups,
                                                                      const int* __restrict__ group_rows, const int4* __restrict__ items,
                                                                      float* __restrict__ ws, int H, int Hkv, long long pre_stride,
                                                                      int pre_tmax, float scale, int nchunk, int sub,
                                                                      const int32_t* __restrict__ n_items_dev, int items_capacity) {
    static_assert(D == 128, "");
    constexpr int KS = D / 32, NT = D / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ln = lane & 15, g = lane >> 4;
    const int head = blockIdx.x * 4 + wave;               // head groups fastest: the (long-first) item list is walked in order
    if (head >= H) return;
    unsigned it = blockIdx.y, n_list = 0;
    if constexpr (LIST) {
        n_list = (unsigned)max(0, min(*n_items_dev, items_capacity));
        if (it >= n_list) return;
    }
    do {            // !LIST: one pass (`continue` leaves it)
        const int4 item = items[LIST ? it : blockIdx.y];
        const GroupDesc gd = groups[item.x];
        // an item = `sub` consecutive 64-key chunks (online softmax across them): one partial per (row, head, item)
        const int r0 = item.y, part = item.z, kbeg = part * ATT_CH * sub;
        if (r0 >= gd.n_rows || kbeg >= gd.plen) continue;
        const int k1 = min(gd.plen, kbeg + ATT_CH * sub);
        const int kvh = head / (H / Hkv);
        // B operand of S^T: this lane's query row
        int rq = r0 + ln; if (rq >= gd.n_rows) rq = gd.n_rows - 1;
        const int qrow = group_rows[gd.row_off + rq];
        frag8_t qf[KS];
        {
            const uint16_t* qp = q + ((size_t)qrow * H + head) * D + g * 8;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const frag8_t*>(qp + ks * 32);
        }
        const uint16_t* fb = frag + 2 * ((size_t)gd.pslot * pre_stride + (size_t)kvh * pre_tmax * D) + (size_t)lane * 8;
        f32x4_t o[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) o[nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        float mrun = -INFINITY, lrun = 0.f;          // of query ln (replicated over g)
        // Chunks in a ROTATED order (the online softmax does not care): every (group, head) stream starts at t = 0 of a region that
        // is a multiple of 32 KiB away from the others', so waves walking in step would all sit on the same HBM channels
        const int nch_i = (k1 - kbeg + ATT_CH - 1) / ATT_CH;
        const int rot = (int)((unsigned)(INVARIANT ? head * 5 + part * 3 : head * 5 + item.x * 3 + r0) % (unsigned)nch_i);
        for (int ci = 0; ci < nch_i; ++ci) {
            const int cc = ci + rot < nch_i ? ci + rot : ci + rot - nch_i;
            const int k0 = kbeg + cc * ATT_CH;
            // The pass is a pure stream (one wave reads the chunk's 32-KiB block and nobody else does), so what matters is bytes in
            // flight: ALL 32 fragment loads of the chunk are issued before the first MFMA.  Issued a few at a time behind their
            // consumers (as the compiler schedules them under a 128-VGPR cap) the pass ran at 4.2 TB/s with 1-2 loads in flight
            // per wave in its P V half.
            frag8_t kf[4][KS], vf[2][NT];
            const uint16_t* cb = fb + (size_t)(k0 / ATT_CH) * FRAG_CHUNK_ELEMS;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) kf[t][ks] = __builtin_nontemporal_load(reinterpret_cast<const frag8_t*>(cb + (t * KS + ks) * 512));
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) vf[kk][nt] = __builtin_nontemporal_load(reinterpret_cast<const frag8_t*>(cb + ATT_CH * D + (kk * NT + nt) * 512));
            __builtin_amdgcn_sched_barrier(0);
            // S^T: 4 tiles (a0, b0 | a1, b1); MFMA row i = ln of the A operand
            f32x4_t s[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                s[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) s[t] = mfma16(kf[t][ks], qf[ks], s[t]);
            }
            // column = query ln; this lane's rows 4 g + r are keys k0 + 32 (t>>1) + 8 g + 4 (t&1) + r
            float mx = -INFINITY;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = k0 + (t >> 1) * 32 + g * 8 + (t & 1) * 4 + r;
                    const float v = key < k1 ? s[t][r] * scale : -INFINITY;
                    s[t][r] = v; mx = fmaxf(mx, v);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16)); mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mnew = fmaxf(mrun, mx);                      // finite: every chunk holds >= 1 valid key
            const float corr = __expf(mrun - mnew);                  // exp(-inf) = 0 on the first chunk
            float lsum = 0.f;
            frag8_t pf[2];
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float pv = __expf(s[kk * 2 + (e >> 2)][e & 3] - mnew);      // exp(-inf) = 0 for masked keys
                    lsum += pv;
                    pf[kk][e] = (short)f2e(pv);
                }
            lsum += __shfl_xor(lsum, 16); lsum += __shfl_xor(lsum, 32);
            lrun = lrun * corr + lsum;
            mrun = mnew;
            if (ci > 0) {           // O rows are queries 4 g + r: their rescale factor lives in the lanes of column 4 g + r
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float cr = __shfl(corr, 4 * g + r);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) o[nt][r] *= cr;
                }
            }
            // O += P V
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                if (k0 + kk * 32 < k1) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) o[nt] = mfma16(pf[kk], vf[kk][nt], o[nt]);
                }
            }
        }
        // O's C layout: column ln of tile nt = dim 8 ln + nt, row = query 4 g + r
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rr = r0 + g * 4 + r;
            if (rr < gd.n_rows) {
                const int orow = group_rows[gd.row_off + rr];
                float* wsp = ws + (((size_t)orow * H + head) * nchunk + part) * ATT_PS + ln * 8;
                *reinterpret_cast<float4*>(wsp) = make_float4(o[0][r], o[1][r], o[2][r], o[3][r]);
                *reinterpret_cast<float4*>(wsp + 4) = make_float4(o[4][r], o[5][r], o[6][r], o[7][r]);
            }
        }
        if (g == 0 && r0 + ln < gd.n_rows) {          // (m, l) of query ln live in the lanes of column ln
            float* wsp = ws + (((size_t)qrow * H + head) * nchunk + part) * ATT_PS;
            *reinterpret_cast<float2*>(wsp + D) = make_float2(mrun, lrun);
        }
    } while (LIST && (it += gridDim.y) < n_list);
}

// the combine pass over a workspace of `nchunk` partials per (row, head), the first `npre` of them prefix items of `pre_keys` keys
static void launch_combine(const void* workspace, const int32_t* rows, void* out, int M, int H, int nchunk, int npre, int pre_keys, hipStream_t st) {
    hipLaunchKernelGGL(decode_attn_combine_kernel<128>, dim3((H + 3) / 4, M), dim3(256), 0, st, (const float*)workspace,
                       (const AttnRow*)rows, (uint16_t*)out, H, nchunk, npre, pre_keys);
}

}  // namespace VDD_ELEM_NS
}  // namespace

using namespace VDD_ELEM_NS;

extern "C" {

VDD_HIDDEN int VDD_IMPL(vdd_decode_attention)(const void* q, const void* k_cache, const void* v_cache, const void* k_prefix, const void* v_prefix,
                         const int32_t* rows, void* out, void* workspace, int M, int H, int Hkv, int D, int64_t slot_stride, int t_max,
                         int64_t prefix_stride, int prefix_tmax, int max_len, float scale, void* stream) {
    if (M <= 0) return VDD_OK;
    if (!q || !k_cache || !v_cache || !k_prefix || !v_prefix || !rows || !out || !workspace || D != 128 || H % Hkv != 0 || max_len <= 0) return VDD_ERR_INVALID_ARG;
    const int nchunk = (max_len + ATT_CH - 1) / ATT_CH;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(decode_attn_kernel<128>, dim3((H + 3) / 4, M, nchunk), dim3(256), 0, st, (const uint16_t*)q,
                       (const uint16_t*)k_cache, (const uint16_t*)v_cache, (const uint16_t*)k_prefix, (const uint16_t*)v_prefix,
                       (const AttnRow*)rows, (float*)workspace, H, Hkv, (long long)slot_stride, t_max, (long long)prefix_stride,
                       prefix_tmax, scale, nchunk, 0, 0);
    launch_combine(workspace, rows, out, M, H, nchunk, 0, ATT_CH, st);
    return ok(hipSuccess);
}

VDD_HIDDEN int VDD_IMPL(vdd_decode_attention_paged)(const void* q, const void* k_pages, const void* v_pages, const int32_t* page_table,
                               const void* k_prefix, const void* v_prefix, const int32_t* rows, void* out, void* workspace, int M, int H,
                               int Hkv, int D, int64_t page_stride, int n_pages, int n_slots, int max_pages_per_slot, int64_t prefix_stride,
                               int prefix_tmax, int max_len, float scale, void* stream) {
    if (M <= 0) return VDD_OK;
    if (!q || !k_prefix || !v_prefix || !rows || !out || !workspace || D != 128 || Hkv <= 0 || H % Hkv != 0 || max_len <= 0 ||
        !paged_args_ok(k_pages, v_pages, page_table, Hkv, D, page_stride, n_pages, n_slots, max_pages_per_slot)) return VDD_ERR_INVALID_ARG;
    const int nchunk = (max_len + ATT_CH - 1) / ATT_CH;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(decode_attn_paged_kernel<128>, dim3((H + 3) / 4, M, nchunk), dim3(256), 0, st, (const uint16_t*)q,
                       (const uint16_t*)k_pages, (const uint16_t*)v_pages, PageTable{page_table, n_slots, max_pages_per_slot, n_pages},
                       (const uint16_t*)k_prefix, (const uint16_t*)v_prefix, (const AttnRow*)rows, (float*)workspace, H, Hkv,
                       (long long)prefix_stride, prefix_tmax, scale, nchunk);
    launch_combine(workspace, rows, out, M, H, nchunk, 0, ATT_CH, st);
    return ok(hipSuccess);
}

VDD_HIDDEN int VDD_IMPL(vdd_decode_attention_fused)(const void* qkv, const int32_t* pos, const int32_t* cpos, const int32_t* slot, const float* cos_sin,
                               void* k_cache, void* v_cache, const void* k_prefix, const void* v_prefix, const int32_t* rows, void* out,
                               int M, int H, int Hkv, int D, int64_t slot_stride, int t_max, int64_t prefix_stride, int prefix_tmax,
                               float scale, void* stream) {
    if (M <= 0) return VDD_OK;
    if (!qkv || !pos || !cpos || !slot || !cos_sin || !k_cache || !v_cache || !k_prefix || !v_prefix || !rows || !out || D != 128 ||
        H % Hkv != 0 || M > 65535) return VDD_ERR_INVALID_ARG;
    hipLaunchKernelGGL((decode_attn_fused_kernel<128, 16, 1>), dim3(H, M), dim3(1024), 0, (hipStream_t)stream, (const uint16_t*)qkv, pos, cpos,
                       slot, cos_sin, (uint16_t*)k_cache, (uint16_t*)v_cache, (const uint16_t*)k_prefix, (const uint16_t*)v_prefix,
                       (const AttnRow*)rows, (uint16_t*)out, H, Hkv, (long long)slot_stride, t_max, (long long)prefix_stride, prefix_tmax,
                       scale, (float*)nullptr, (int*)nullptr);
    return ok(hipSuccess);
}

VDD_HIDDEN int64_t VDD_IMPL(vdd_decode_attention_fused_split_workspace_bytes)(int M, int H, int n_split) {
    if (M <= 0 || H <= 0 || n_split < 1) return 0;
    return ((int64_t)M * H * n_split * ATT_FS + (int64_t)M * H) * 4;
}

VDD_HIDDEN int VDD_IMPL(vdd_decode_attention_fused_split)(const void* qkv, const int32_t* pos, const int32_t* cpos, const int32_t* slot, const float* cos_sin,
                                     void* k_cache, void* v_cache, const void* k_prefix, const void* v_prefix, const int32_t* rows, void* out,
                                     int M, int H, int Hkv, int D, int64_t slot_stride, int t_max, int64_t prefix_stride, int prefix_tmax,
                                     float scale, void* workspace, int n_split, void* stream) {
    if (M <= 0) return VDD_OK;
    if (!qkv || !pos || !cpos || !slot || !cos_sin || !k_cache || !v_cache || !k_prefix || !v_prefix || !rows || !out || !workspace || D != 128 ||
        H % Hkv != 0 || M > 65535 || (n_split != 2 && n_split != 4)) return VDD_ERR_INVALID_ARG;
    float* ws = (float*)workspace;
    int* tickets = (int*)(ws + (size_t)M * H * n_split * ATT_FS);
#define VDD_FUSED_SPLIT(KS)                                                                                                            \
    hipLaunchKernelGGL((decode_attn_fused_kernel<128, 16, KS>), dim3(H, M, KS), dim3(1024), 0, (hipStream_t)stream, (const uint16_t*)qkv, pos, \
                       cpos, slot, cos_sin, (uint16_t*)k_cache, (uint16_t*)v_cache, (const uint16_t*)k_prefix, (const uint16_t*)v_prefix,  \
                       (const AttnRow*)rows, (uint16_t*)out, H, Hkv, (long long)slot_stride, t_max, (long long)prefix_stride, prefix_tmax, \
                       scale, ws, tickets)
    if (n_split == 2) VDD_FUSED_SPLIT(2); else VDD_FUSED_SPLIT(4);
#undef VDD_FUSED_SPLIT
    return ok(hipSuccess);
}

VDD_HIDDEN int VDD_IMPL(vdd_decode_attention_grouped)(const void* q, const void* k_cache, const void* v_cache, const void* k_prefix, const void* v_prefix,
                                 const void* prefix_frag, const int32_t* rows, const int32_t* groups, const int32_t* group_rows,
                                 const int32_t* items, int n_items, void* out, void* workspace, int M, int H, int Hkv, int D,
                                 int64_t slot_stride, int t_max, int64_t prefix_stride, int prefix_tmax, int max_prefix_len,
                                 int max_own_len, int prefix_chunks_per_item, float scale, void* stream) {
    if (M <= 0) return VDD_OK;
    if (!q || !k_cache || !v_cache || !k_prefix || !v_prefix || !rows || !groups || !group_rows || !items || !out || !workspace || D != 128 ||
        H % Hkv != 0 || max_own_len <= 0 || max_prefix_len < 0 || n_items < 0 || n_items > 65535 || prefix_chunks_per_item < 1) return VDD_ERR_INVALID_ARG;
    if (n_items > 0 && (prefix_frag == nullptr || prefix_tmax % ATT_CH != 0)) return VDD_ERR_INVALID_ARG;     // the MFMA prefix pass reads the fragment-major image
    const int sub = prefix_chunks_per_item;                                     // it leaves one partial per item of `sub` 64-key chunks
    const int pre_keys = ATT_CH * sub;
    const int npre = (max_prefix_len + pre_keys - 1) / pre_keys, nown = (max_own_len + ATT_CH - 1) / ATT_CH;
    const int nchunk = npre + nown;
    hipStream_t st = (hipStream_t)stream;
    if (n_items > 0 && npre > 0) {
        hipLaunchKernelGGL(decode_attn_prefix_mfma_kernel<128>, dim3((H + 3) / 4, n_items), dim3(256), 0, st,
                           (const uint16_t*)q, (const uint16_t*)prefix_frag, (const GroupDesc*)groups, group_rows,
                           (const int4*)items, (float*)workspace, H, Hkv, (long long)prefix_stride, prefix_tmax, scale, nchunk, sub,
                           (const int32_t*)nullptr, 0);
    }
    if (max_own_len <= 256) {        // short own ranges: one wave per (row, head) finishes the row (own keys + prefix partials)
        hipLaunchKernelGGL(decode_attn_own_merge_kernel<128>, dim3((H + 3) / 4, M), dim3(256), 0, st, (const uint16_t*)q,
                           (const uint16_t*)k_cache, (const uint16_t*)v_cache, (const AttnRow*)rows, (const float*)workspace,
                           (uint16_t*)out, H, Hkv, (long long)slot_stride, t_max, scale, nchunk, npre, pre_keys);
        return ok(hipSuccess);
    }
    hipLaunchKernelGGL(decode_attn_kernel<128>, dim3((H + 3) / 4, M, nown), dim3(256), 0, st, (const uint16_t*)q,
                       (const uint16_t*)k_cache, (const uint16_t*)v_cache, (const uint16_t*)k_prefix, (const uint16_t*)v_prefix,
                       (const AttnRow*)rows, (float*)workspace, H, Hkv, (long long)slot_stride, t_max, (long long)prefix_stride,
                       prefix_tmax, scale, nchunk, 1, npre);
    launch_combine(workspace, rows, out, M, H, nchunk, npre, pre_keys, st);
    return ok(hipSuccess);
}

VDD_HIDDEN int VDD_IMPL(vdd_decode_attention_shared_invariant)(const void* q, const void* k_cache, const void* v_cache, const void* k_prefix,
                                          const void* v_prefix, const void* prefix_frag, const int32_t* rows, const int32_t* row_mode,
                                          const int32_t* groups, const int32_t* group_rows, const int32_t* items, int n_items, void* out,
                                          void* workspace, int M, int H, int Hkv, int D, int64_t slot_stride, int t_max,
                                          int64_t prefix_stride, int prefix_tmax, int max_prefix_len, int max_own_len, int max_row_len,
                                          int prefix_chunks_per_item, float scale, void* stream) {
    if (M <= 0) return VDD_OK;
    if (!q || !k_cache || !v_cache || !k_prefix || !v_prefix || !rows || !row_mode || !groups || !group_rows || !items || !out || !workspace ||
        D != 128 || Hkv <= 0 || H % Hkv != 0 || max_prefix_len < 0 || max_own_len < 0 || max_row_len < 0 || max_own_len + max_row_len <= 0 ||
        n_items < 0 || n_items > 65535 || prefix_chunks_per_item < 1) return VDD_ERR_INVALID_ARG;
    if (n_items > 0 && (prefix_frag == nullptr || prefix_tmax % ATT_CH != 0)) return VDD_ERR_INVALID_ARG;
    const int sub = prefix_chunks_per_item, pre_keys = ATT_CH * sub;
    const int npre = (max_prefix_len + pre_keys - 1) / pre_keys, nown = (max_own_len + ATT_CH - 1) / ATT_CH, nrow = (max_row_len + ATT_CH - 1) / ATT_CH;
    const int nchunk = npre + nown > nrow ? npre + nown : nrow;
    hipStream_t st = (hipStream_t)stream;
    if (n_items > 0 && npre > 0) {
        hipLaunchKernelGGL((decode_attn_prefix_mfma_kernel<128, true>), dim3((H + 3) / 4, n_items), dim3(256), 0, st,
                           (const uint16_t*)q, (const uint16_t*)prefix_frag, (const GroupDesc*)groups, group_rows,
                           (const int4*)items, (float*)workspace, H, Hkv, (long long)prefix_stride, prefix_tmax, scale, nchunk, sub,
                           (const int32_t*)nullptr, 0);
    }
    hipLaunchKernelGGL(decode_attn_mixed_kernel<128>, dim3((H + 3) / 4, M, nown > nrow ? nown : nrow), dim3(256), 0, st, (const uint16_t*)q,
                       (const uint16_t*)k_cache, (const uint16_t*)v_cache, (const uint16_t*)k_prefix, (const uint16_t*)v_prefix,
                       (const AttnRow*)rows, row_mode, (float*)workspace, H, Hkv, (long long)slot_stride, t_max, (long long)prefix_stride,
                       prefix_tmax, scale, nchunk, npre, nown, nrow);
    hipLaunchKernelGGL(decode_attn_combine_mixed_kernel<128>, dim3((H + 3) / 4, M), dim3(256), 0, st, (const float*)workspace,
                       (const AttnRow*)rows, row_mode, (uint16_t*)out, H, nchunk, npre, pre_keys);
    return ok(hipSuccess);
}

// blocks of the list form's prefix pass: enough to keep every CU of the chip busy several times over (the items are walked with a stride),
// never more than the list can hold
constexpr int PREFIX_LIST_BLOCKS = 2048;
static int prefix_list_grid_y(int items_capacity, int H) {
    const int by_chip = (PREFIX_LIST_BLOCKS + (H + 3) / 4 - 1) / ((H + 3) / 4);
    return items_capacity < by_chip ? items_capacity : by_chip;
}

VDD_HIDDEN int VDD_IMPL(vdd_decode_attention_grouped_list)(const void* q, const void* k_cache, const void* v_cache, const int32_t* page_table,
                                      const void* k_prefix, const void* v_prefix, const void* prefix_frag, const int32_t* rows,
                                      const int32_t* groups, const int32_t* group_rows, const int32_t* items, const int32_t* n_items_dev,
                                      int items_capacity, void* out, void* workspace, int M, int H, int Hkv, int D, int64_t slot_stride,
                                      int t_max, int n_pages, int n_slots, int max_pages_per_slot, int64_t prefix_stride, int prefix_tmax,
                                      int max_prefix_len, int max_own_len, int prefix_chunks_per_item, float scale, void* stream) {
    if (M <= 0) return VDD_OK;
    if (!q || !k_cache || !v_cache || !k_prefix || !v_prefix || !rows || !groups || !group_rows || !items || !out || !workspace || D != 128 ||
        Hkv <= 0 || H % Hkv != 0 || max_own_len <= 0 || max_prefix_len < 0 || prefix_chunks_per_item < 1) return VDD_ERR_INVALID_ARG;
    if (!n_items_dev || items_capacity < 1 || items_capacity > 65535) return VDD_ERR_INVALID_ARG;
    if (prefix_frag == nullptr || prefix_tmax % ATT_CH != 0) return VDD_ERR_INVALID_ARG;      // the list may hold items at any replay
    if (page_table && !paged_args_ok(k_cache, v_cache, page_table, Hkv, D, slot_stride, n_pages, n_slots, max_pages_per_slot)) return VDD_ERR_INVALID_ARG;
    const int sub = prefix_chunks_per_item, pre_keys = ATT_CH * sub;
    const int npre = (max_prefix_len + pre_keys - 1) / pre_keys, nown = (max_own_len + ATT_CH - 1) / ATT_CH;
    const int nchunk = npre + nown;
    hipStream_t st = (hipStream_t)stream;
    const PageTable pt{page_table, n_slots, max_pages_per_slot, n_pages};
    if (npre > 0) {
        hipLaunchKernelGGL((decode_attn_prefix_mfma_kernel<128, false, true>), dim3((H + 3) / 4, prefix_list_grid_y(items_capacity, H)), dim3(256), 0, st,
                           (const uint16_t*)q, (const uint16_t*)prefix_frag, (const GroupDesc*)groups, group_rows, (const int4*)items,
                           (float*)workspace, H, Hkv, (long long)prefix_stride, prefix_tmax, scale, nchunk, sub, n_items_dev, items_capacity);
    }
    if (max_own_len <= 256) {
        if (page_table)
            hipLaunchKernelGGL(decode_attn_own_merge_paged_kernel<128>, dim3((H + 3) / 4, M), dim3(256), 0, st, (const uint16_t*)q,
                               (const uint16_t*)k_cache, (const uint16_t*)v_cache, pt, (const AttnRow*)rows, (const float*)workspace,
                               (uint16_t*)out, H, Hkv, scale, nchunk, npre, pre_keys);
        else
            hipLaunchKernelGGL(decode_attn_own_merge_kernel<128>, dim3((H + 3) / 4, M), dim3(256), 0, st, (const uint16_t*)q,
                               (const uint16_t*)k_cache, (const uint16_t*)v_cache, (const AttnRow*)rows, (const float*)workspace,
                               (uint16_t*)out, H, Hkv, (long long)slot_stride, t_max, scale, nchunk, npre, pre_keys);
        return ok(hipSuccess);
    }
    if (page_table)
        hipLaunchKernelGGL(decode_attn_paged_own_kernel<128>, dim3((H + 3) / 4, M, nown), dim3(256), 0, st, (const uint16_t*)q,
                           (const uint16_t*)k_cache, (const uint16_t*)v_cache, pt, (const uint16_t*)k_prefix, (const uint16_t*)v_prefix,
                           (const AttnRow*)rows, (float*)workspace, H, Hkv, (long long)prefix_stride, prefix_tmax, scale, nchunk, npre);
    else
        hipLaunchKernelGGL(decode_attn_kernel<128>, dim3((H + 3) / 4, M, nown), dim3(256), 0, st, (const uint16_t*)q,
                           (const uint16_t*)k_cache, (const uint16_t*)v_cache, (const uint16_t*)k_prefix, (const uint16_t*)v_prefix,
                           (const AttnRow*)rows, (float*)workspace, H, Hkv, (long long)slot_stride, t_max, (long long)prefix_stride,
                           prefix_tmax, scale, nchunk, 1, npre);
    launch_combine(workspace, rows, out, M, H, nchunk, npre, pre_keys, st);
    return ok(hipSuccess);
}

VDD_HIDDEN int VDD_IMPL(vdd_decode_attention_shared_invariant_list)(const void* q, const void* k_cache, const void* v_cache, const void* k_prefix,
                                               const void* v_prefix, const void* prefix_frag, const int32_t* rows, const int32_t* row_mode,
                                               const int32_t* groups, const int32_t* group_rows, const int32_t* items,
                                               const int32_t* n_items_dev, int items_capacity, void* out, void* workspace, int M, int H,
                                               int Hkv, int D, int64_t slot_stride, int t_max, int64_t prefix_stride, int prefix_tmax,
                                               int max_prefix_len, int max_own_len, int max_row_len, int prefix_chunks_per_item, float scale,
                                               void* stream) {
    if (M <= 0) return VDD_OK;
    if (!q || !k_cache || !v_cache || !k_prefix || !v_prefix || !rows || !row_mode || !groups || !group_rows || !items || !out || !workspace ||
        D != 128 || Hkv <= 0 || H % Hkv != 0 || max_prefix_len < 0 || max_own_len < 0 || max_row_len < 0 || max_own_len + max_row_len <= 0 ||
        prefix_chunks_per_item < 1) return VDD_ERR_INVALID_ARG;
    if (!n_items_dev || items_capacity < 1 || items_capacity > 65535) return VDD_ERR_INVALID_ARG;
    if (prefix_frag == nullptr || prefix_tmax % ATT_CH != 0) return VDD_ERR_INVALID_ARG;
    const int sub = prefix_chunks_per_item, pre_keys = ATT_CH * sub;
    const int npre = (max_prefix_len + pre_keys - 1) / pre_keys, nown = (max_own_len + ATT_CH - 1) / ATT_CH, nrow = (max_row_len + ATT_CH - 1) / ATT_CH;
    const int nchunk = npre + nown > nrow ? npre + nown : nrow;
    hipStream_t st = (hipStream_t)stream;
    if (npre > 0) {
        hipLaunchKernelGGL((decode_attn_prefix_mfma_kernel<128, true, true>), dim3((H + 3) / 4, prefix_list_grid_y(items_capacity, H)), dim3(256), 0, st,
                           (const uint16_t*)q, (const uint16_t*)prefix_frag, (const GroupDesc*)groups, group_rows, (const int4*)items,
                           (float*)workspace, H, Hkv, (long long)prefix_stride, prefix_tmax, scale, nchunk, sub, n_items_dev, items_capacity);
    }
    hipLaunchKernelGGL(decode_attn_mixed_kernel<128>, dim3((H + 3) / 4, M, nown > nrow ? nown : nrow), dim3(256), 0, st, (const uint16_t*)q,
                       (const uint16_t*)k_cache, (const uint16_t*)v_cache, (const uint16_t*)k_prefix, (const uint16_t*)v_prefix,
                       (const AttnRow*)rows, row_mode, (float*)workspace, H, Hkv, (long long)slot_stride, t_max, (long long)prefix_stride,
                       prefix_tmax, scale, nchunk, npre, nown, nrow);
    hipLaunchKernelGGL(decode_attn_combine_mixed_kernel<128>, dim3((H + 3) / 4, M), dim3(256), 0, st, (const float*)workspace,
                       (const AttnRow*)rows, row_mode, (uint16_t*)out, H, nchunk, npre, pre_keys);
    return ok(hipSuccess);
}

VDD_HIDDEN int VDD_IMPL(vdd_prefix_fragments)(const void* k_prefix, const void* v_prefix, void* prefix_frag, const int32_t* prefix_len_of_slot, int n_slots,
                         int Hkv, int t_max, int D, void* stream) {
    if (n_slots <= 0) return VDD_OK;
    if (!k_prefix || !v_prefix || !prefix_frag || !prefix_len_of_slot || D != 128 || t_max % ATT_CH != 0) return VDD_ERR_INVALID_ARG;
    hipLaunchKernelGGL(prefix_fragments_kernel, dim3(t_max / ATT_CH, Hkv, n_slots), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)k_prefix, (const uint16_t*)v_prefix, (uint16_t*)prefix_frag, t_max, prefix_len_of_slot);
    return ok(hipSuccess);
}

VDD_HIDDEN int64_t VDD_IMPL(vdd_decode_attention_workspace_bytes)(int M, int H, int D, int max_len) {
    return (int64_t)M * H * ((max_len + ATT_CH - 1) / ATT_CH) * ATT_PS * 4;
}

}  // extern "C"
