// abi_common.hip -- version, device probe and error reporting of the C ABI.
#include "abi_common.hpp"
#include "../../include/iago_hip_serving.h" // (iago_gumbel_root)

#include <stdio.h>
#include <string.h>
#include <string>

namespace {
thread_local char g_err[512] = "";
}

int iago_fail(int code, const char *msg)
{
    snprintf(g_err, sizeof g_err, "%s", msg);
    return code;
}

int iago_check_gumbel_root(const iago_gumbel_root *gz, const char *who)
{
    const std::string w(who);
    if (!gz)
        return iago_fail(IAGO_ERR_INVALID, (w + ": null gumbel arguments").c_str());
    if (gz->reserved0 != 0)
        return iago_fail(IAGO_ERR_INVALID, (w + ": reserved fields must be 0").c_str());
    if (gz->m < 2 || gz->m > 64)
        return iago_fail(IAGO_ERR_INVALID, (w + ": m must be in [2, 64]").c_str());
    if (gz->c_scale_256 < 1 || gz->c_scale_256 > 4096)
        return iago_fail(IAGO_ERR_INVALID, (w + ": c_scale_256 must be in [1, 4096]").c_str());
    if (gz->c_visit < 0 || gz->c_visit > 4096)
        return iago_fail(IAGO_ERR_INVALID, (w + ": c_visit must be in [0, 4096]").c_str());
    if (!gz->gumbel_q16 || !gz->ln_q16 || !gz->g)
        return iago_fail(IAGO_ERR_INVALID, (w + ": null table or draws buffer (gumbel_q16, ln_q16 and g expected)").c_str());
    return IAGO_OK;
}

int iago_check_launch(const char *where)
{
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        return IAGO_OK;
    snprintf(g_err, sizeof g_err, "%s: %s", where, hipGetErrorString(e));
    return IAGO_ERR_HIP;
}

int iago_reserve_lds(const void *kernel, int bytes, std::atomic<uint64_t> &done, const char *who)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return iago_fail(IAGO_ERR_HIP, who);
    }
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit)
        return IAGO_OK;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return iago_fail(IAGO_ERR_HIP, who);
    }
    done.fetch_or(bit, std::memory_order_release);
    return IAGO_OK;
}

int iago_device_cus()
{
    static std::atomic<int> cus{0};
    int c = cus.load(std::memory_order_relaxed);
    if (c > 0)
        return c;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) !=
                                                 hipSuccess || c <= 0) {
        (void)hipGetLastError();
        return 0;
    }
    cus.store(c, std::memory_order_relaxed);
    return c;
}

static int search_fail(const char *who, const char *what, const char *name)
{
    char msg[128];
    snprintf(msg, sizeof msg, "%s: %s%s", who, what, name);
    return iago_fail(IAGO_ERR_HIP, msg);
}

int iago_search_prepare(const char *who, uint32_t *ctl, int ctl_words, uint8_t *done, const char *done_name, int64_t n,
                        hipStream_t s, int *cus)
{
    *cus = 0;
    if (hipMemsetAsync(ctl, 0, ctl_words * sizeof(uint32_t), s) != hipSuccess) {
        (void)hipGetLastError();
        return search_fail(who, "clearing ", "ctl");
    }
    if (n == 0)
        return IAGO_OK;
    if (done && hipMemsetAsync(done, 0, (size_t)n, s) != hipSuccess) {
        (void)hipGetLastError();
        return search_fail(who, "clearing ", done_name);
    }
    *cus = iago_device_cus();
    if (*cus <= 0)
        return search_fail(who, "no HIP device", "");
    return IAGO_OK;
}

void iago_search_launch(const void *kernel, void *params, int levels, int frame_bytes, int64_t lanes, int cus,
                        hipStream_t s)
{
    const int wave = 64;
    const int lds = levels * wave * frame_bytes;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, wave, lds) != hipSuccess || per_cu <= 0) {
        (void)hipGetLastError();
        per_cu = 1;
    }
    const int64_t want = (lanes + wave - 1) / wave;
    const int64_t cap = (int64_t)cus * per_cu;
    const unsigned grid = (unsigned)(want < cap ? want : cap);
    void *args[] = {params};
    if (grid > 0)
        (void)hipLaunchKernel(kernel, dim3(grid), dim3(wave), args, lds, s); // (an error stays for iago_check_launch)
}

extern "C" {

int iago_abi_version(void) { return 13; }

const char *iago_last_error(void) { return g_err; }

int iago_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

} // extern "C"
