// What the two decode-step translation units (vdd_llm_kernels.hip, vdd_decode_attention.hip) share: the 16-byte fragment type, the
// nontemporal load / store helpers, the packed dot product, the page table of the paged own-KV pool and the entries' common host
// checks.  Like them it is compiled once per storage type (csrc/vdd_elem.h), inside that instantiation's namespace.
#ifndef VDD_LLM_COMMON_H
#define VDD_LLM_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vdd_elem.h"

namespace {
namespace VDD_ELEM_NS {
using namespace vdd_elem;

typedef __attribute__((ext_vector_type(8))) short frag8_t;    // MFMA A/B fragment: 8 elements (bf16 or fp16 bit patterns)
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_nt;
// data that crosses the chip once (an activation read by one kernel, a cache line written for a later step): nontemporal, so it
// takes no L2 line from data that IS re-read (the GEMMs' shared operand panels, the next GEMM's X)
__device__ __forceinline__ uint4 ld_stream(const uint16_t* p) { return __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4_nt*>(p))); }
__device__ __forceinline__ void st_stream(uint16_t* p, uint4 v) { __builtin_nontemporal_store(__builtin_bit_cast(u32x4_nt, v), reinterpret_cast<u32x4_nt*>(p)); }

// q.k over 8 packed pairs with v_dot2c_f32_{bf16,f16} (fp32 accumulate; the 16-bit x 16-bit products are exact in fp32)
__device__ __forceinline__ float dot8(const uint4& a, const uint4& b) {
    float s = dot2(a.x, b.x, 0.f);
    s = dot2(a.y, b.y, s);
    s = dot2(a.z, b.z, s);
    s = dot2(a.w, b.w, s);
    return s;
}

// Paged own-KV pool (engine.generate_list(paged_kv=True)): pools [n_pages, Hkv, KV_PAGE, D]; own token i of own slot s lives in page
// table[s][i / KV_PAGE] at index i % KV_PAGE.
constexpr int KV_PAGE = VDD_KV_PAGE;
struct PageTable { const int* table; int n_slots, max_pages, n_pages; };
// page of own token i of slot s, or -1
__device__ __forceinline__ int page_of(const PageTable& pt, int s, int i) {
    const int pi = i / KV_PAGE;
    if (s < 0 || s >= pt.n_slots || i < 0 || pi >= pt.max_pages) return -1;
    const int pg = pt.table[(size_t)s * pt.max_pages + pi];
    return pg < pt.n_pages ? pg : -1;
}

inline int ok(hipError_t) { return hipGetLastError() == hipSuccess ? VDD_OK : VDD_ERR_LAUNCH; }

// what the three paged entries check before any launch: a dense page pool and a table that can be indexed
inline bool paged_args_ok(const void* k_pages, const void* v_pages, const int32_t* page_table, int Hkv, int D, int64_t page_stride, int n_pages,
                          int n_slots, int max_pages_per_slot) {
    return k_pages && v_pages && page_table && Hkv > 0 && D > 0 && D % 8 == 0 && n_pages > 0 && n_slots > 0 && max_pages_per_slot > 0 &&
           page_stride == (int64_t)Hkv * KV_PAGE * D;
}

}  // namespace VDD_ELEM_NS
}  // namespace

#endif /* VDD_LLM_COMMON_H */
