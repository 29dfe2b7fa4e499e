// last_search.h — what the last user-facing search of a context left to be read back (zvec_hip_ctx_last_route, _last_ivf_plan,
// zvec_hip_ivf_last_stats, zvec_hip_bivf_last_probes / _last_candidates, zvec_hip_*hnsw*_last_stats, the certify step of the half-width
// pre-selection): one record per context, host numbers only — the device buffers they describe stay where they are.  DESIGN §3
// "What a search leaves on its context".  Nothing of HIP: tests/cpp/test_last_search_cpu.cc.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>

#include "../../../include/zvec_hip.h"      // (ZVEC_HIP_IVF_ROUTE_*)

// What an IVF search planned: the route it took and where its arrays lie inside the context's plan buffer (u32 word offsets: the
// buffer may be reallocated, the offsets hold).  Both direct routes keep q_nprobe and q_scanned there, the tile route every array
// (`words` != 0), the large-k route none.
struct IvfPlanMark {
  uint32_t route = 0;                      // ZVEC_HIP_IVF_ROUTE_*; 0 = the search planned nothing that can be read back
  uint32_t scan_threads = 0;               // threads of plan_scan_kernel (tile route)
  uint32_t nq = 0, nlist = 0, nprobe = 0;  // nprobe: probe ranks per query (nlist under brute force)
  uint32_t tpc = 0, rows_per_group = 0, brute_force = 0;
  uint64_t slots_bound = 0;                // what part_s / part_i were sized from
  uint64_t npairs = 0;                     // capacity of csr_q / csr_slot
  size_t words = 0;                        // words of the plan buffer in use (tile route)
  size_t o_qnprobe = 0, o_qscanned = 0, o_qnslots = 0, o_slotbegin = 0, o_lcount = 0, o_lqoff = 0, o_itemoff = 0, o_ltpc = 0,
         o_total = 0, o_csrq = 0, o_csrslot = 0;
  bool has_stats() const { return route != ZVEC_HIP_IVF_ROUTE_NONE && route != ZVEC_HIP_IVF_ROUTE_LARGE_K; }
};

// The record belongs to the LAST user-facing search of the context.  Such a search calls begin() once, before it enqueues anything:
// whatever an earlier search left — of any family, on any handle — is gone.  It writes its own family's marks as it goes and sets
// `count` when all of its work is enqueued; until then (and after a search that failed half-way) no reader is admitted.  Passes inside
// a search (the IVF coarse pass and the seeding prefix through the flat scan, the slices of a batch) never begin: they only OR into
// `route`, which nobody can read under another family.  The certify step takes its numbers first (take_certify); the searches it
// re-runs are user-facing searches of the same handle and begin again.  Only touched under the context's mutex.
struct LastSearch {
  enum Family : uint32_t { NONE = 0, FLAT, IVF, HAMMING_IVF, HNSW, SPARSE };
  Family family = NONE;
  const void *owner = nullptr;             // the index handle
  uint32_t count = 0;                      // queries whose marks can be read back
  uint32_t route = 0;                      // FLAT: ROUTE_* of what the search launched (api_flat_scan.inc.h)
  IvfPlanMark ivf;                         // IVF: of the last slice of the batch
  uint32_t bivf_np = 0;                    // HAMMING_IVF: row stride of the probe lists ...
  uint32_t bivf_cand_kc = 0, bivf_cand_slice = 0;      // ... and of stage 1 of a search with fp32 re-ranking (kc 0: none)
  uint32_t hnsw_slices = 0;                // HNSW, dense and sparse: slices the batch went in
  struct Certify {                         // FLAT, IVF: the certify step a search through the fp16 twin leaves pending
    uint32_t count = 0, kp = 0, topk = 0;  // queries (0: none pending), pre-selection width, k
  } certify;

  void begin(Family f, const void *h) {
    *this = LastSearch();
    family = f;
    owner = h;
  }
  // is the context's last search one of family f by handle h with at least n queries?
  bool admits(Family f, const void *h, uint32_t n) const { return f != NONE && family == f && owner == h && count != 0 && n <= count; }
  // the two readers that take no handle
  uint32_t flat_route() const { return family == FLAT ? route : 0u; }
  IvfPlanMark ivf_plan() const { return family == IVF ? ivf : IvfPlanMark(); }
  // the pending certify step leaves the record with its taker
  Certify take_certify() { return std::exchange(certify, Certify()); }
};
