// zvec_hip_api.hip — host side of the C ABI in include/zvec_hip.h: HBM-resident stores, search
// orchestration (prep -> [coarse -> plan] -> scan -> merge), IVF build, and the measurement hook.
// gfx950 only; no CPU fallback exists anywhere in this file: if HIP is unavailable the calls fail.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <sched.h>
#include <time.h>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <shared_mutex>
#include <new>
#include <vector>

#include "../../include/zvec_hip.h"
#include "scan_kernels.hip.h"
#include "host/hole_bits.h"
#include "host/sparse_put_plan.h"
#include "host/ivf_layout.h"
#include "host/hnsw_add_plan.h"

using namespace zvk;

#include "api_types.inc.h"
#include "api_flat_scan.inc.h"
#include "api_ivf_core.inc.h"

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

#include "api_entry_ctx_flat.inc.h"
#include "api_entry_ivf.inc.h"
#include "api_entry_merge_prof.inc.h"
#include "api_entry_filter.inc.h"
#include "api_entry_binary_quant.inc.h"
#include "api_entry_hamming_ivf.inc.h"
#include "api_entry_hamming_ivf_fp32.inc.h"
#include "api_entry_group.inc.h"
#include "api_entry_shards.inc.h"
#include "api_entry_container.inc.h"
#include "api_entry_sparse.inc.h"
#include "api_entry_sparse_put.inc.h"
#include "api_entry_sparse_inverted.inc.h"
#include "api_entry_sparse_ingest.inc.h"
#include "api_entry_sparse_put_dev.inc.h"
#include "api_entry_sparse_group.inc.h"
#include "api_entry_hnsw.inc.h"
#include "api_entry_hnsw_build.inc.h"
#include "api_entry_hnsw_add.inc.h"

}  // extern "C"
