// Host-side plumbing every file with extern "C" entry points shares (defined in host.hip): the
// thread's error message, the mbrl_set_option switches, the shape -> Geometry check.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/mbrl_cem.h"
#include "mbrl_internal.h"

namespace mbrl {

// Sets the calling thread's mbrl_last_error() text and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// MBRL_OK, or MBRL_EHIP with "<what>: <HIP's error string>".
int hip_check(hipError_t e, const char* what);

// The value of an mbrl_set_option switch (include/mbrl_cem.h MBRL_OPT_*); 0 = automatic.
int opt(int option);

// traj_coop_kernel / gd_coop_kernel hand-off mode under MBRL_OPT_TRAJ_HOP / MBRL_OPT_GD_HOP = 0
// (TrajArgs.hop_mode)
constexpr int kTrajHopDefault = 2;

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The Geometry of an ABI shape; MBRL_EINVAL / MBRL_EUNSUPPORTED with the message set.
int shape_geometry(const mbrl_mlp_shape* sh, Geometry* g);

}  // namespace mbrl
