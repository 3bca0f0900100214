// abi_common.hpp -- error plumbing shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/iago_hip_experimental.h" // (includes iago_hip.h)

// Records `msg` as the thread's last error and returns `code`.
int iago_fail(int code, const char *msg);
// hipGetLastError() after a launch -> IAGO_OK / IAGO_ERR_HIP.
int iago_check_launch(const char *where);

// The arguments of the Gumbel root search (iago_gumbel_root, include/iago_hip_serving.h) as the three entry points that take
// them check them: null, reserved0, m in [2, 64], c_scale_256 in [1, 4096], c_visit in [0, 4096], the two tables and g.
// `who`: the entry point, which the refusal's text begins with.  IAGO_OK or IAGO_ERR_INVALID.
struct iago_gumbel_root;
int iago_check_gumbel_root(const iago_gumbel_root *gz, const char *who);

// The current device's compute units (asked once per process); 0 when there is no HIP device.
int iago_device_cus();

// The host side of a lane-per-position search launch (lane_search.hpp), in two steps so that a caller may enqueue
// stages of its own between them.  iago_search_prepare: ctl's first ctl_words words cleared; n == 0: IAGO_OK with
// *cus = 0, there is nothing to launch; else the n bytes of `done` cleared (a null `done` is skipped) and the device's
// compute units in *cus.  Errors are recorded as "<who>: clearing ctl", "<who>: clearing <done_name>",
// "<who>: no HIP device".
int iago_search_prepare(const char *who, uint32_t *ctl, int ctl_words, uint8_t *done, const char *done_name, int64_t n,
                        hipStream_t s, int *cus);
// iago_search_launch: `kernel` (one wave per workgroup, one params struct, levels x 64 x frame_bytes of dynamic LDS)
// with a lane per `lanes`, but never more workgroups than the CUs hold at once -- the give-up is per wave's own
// clock, so every workgroup must be resident.  No launch for lanes == 0.  The caller asks iago_check_launch.
void iago_search_launch(const void *kernel, void *params, int levels, int frame_bytes, int64_t lanes, int cus,
                        hipStream_t s);

#include <atomic>
// One-time hipFuncSetAttribute(MaxDynamicSharedMemorySize) per (kernel, device): `done` is a
// per-kernel bit mask of the devices already configured.  Safe from several threads (a lost
// race only repeats an idempotent call).  Returns IAGO_OK or IAGO_ERR_HIP.
int iago_reserve_lds(const void *kernel, int bytes, std::atomic<uint64_t> &done, const char *who);
