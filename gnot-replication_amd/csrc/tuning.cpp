// The plan's tuning switches (gnot_kernels.h Tuning): the one place that reads them from the environment.
// GNOT_LINEAR_OC (linear.hip) and GNOT_LINEAR2_CHUNKS (linear2.hip) are not here: they stay process-wide.
#include <cstdlib>

#include "gnot_kernels.h"

namespace gnot {

Tuning tuning_from_env() {
  Tuning t;
  if (const char* e = std::getenv("GNOT_WGRAD_OVERLAP")) t.wgrad_overlap = e[0] == '1' ? 1 : 0;
  if (const char* e = std::getenv("GNOT_MOE_STORED_STREAMS")) t.moe_stored = e[0] == '1';
  if (const char* e = std::getenv("GNOT_STATE_MFMA_MIN")) t.state_mfma_min_points = std::atol(e);
  if (const char* e = std::getenv("GNOT_APPLY_MFMA_MIN")) t.apply_mfma_min_chunks = std::atoi(e);
  return t;
}

}  // namespace gnot
