// powder_play.h -- what play.hip (include/ogbx_play.h) needs of powder.hip:
// the data-collection reset of a powder handle, whose kernels use the world
// code of powder.hip / powder_full.h.  Internal to libogbx.
#pragma once

#include "common.h"

namespace ogbx {

// ogbx_play_powder_reset after its NULL checks (env and obs are non-NULL).
__attribute__((visibility("hidden"))) ogbx_status powder_data_reset(ogbx_powder_t env, const uint8_t* mask,
                                                                    uint8_t* obs, uint64_t seed, void* stream);

}  // namespace ogbx
