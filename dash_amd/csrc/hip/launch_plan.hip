// Launch planning state shared by every kernel unit (declared in launch.h): the CU count the launch pickers plan
// with, and the launch log.
//
// The planning count is the device's CU count unless a test has set an override (set_planning_cus; no environment
// variable reads it). It decides only WHICH form of a gadget kernel is launched and with what block size and grid
// (gadget_common.h aes_bs / aes_block_cap, mrs_chain.h mrs_staged / mrs_wave_lds, kernels_gadget.hip out_quad_fits /
// launch_relu_mult / launch_rescale_update_approx). It does not move work: every launch still goes to the stream's
// device and uses all of its CUs. The pickers' correctness preconditions (N % 16 == 0, N >= block, mrs_odd_base,
// the 160 KiB LDS bound, n <= 128) do not depend on it.
#include <cstdio>

#include "launch.h"

namespace dash {
namespace dev {

namespace {
std::atomic<int> g_planning_cus{0};  // 0: the device's count
std::mutex g_log_mu;
std::vector<std::string> g_log;

int device_cus() {
    static int cus = [] {
        int dev = 0, n = 256;
        if (hipGetDevice(&dev) == hipSuccess) hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        return n;
    }();
    return cus;
}
}  // namespace

std::atomic<bool> g_launch_log_on{false};

int num_cus() {
    const int o = g_planning_cus.load(std::memory_order_relaxed);
    return o > 0 ? o : device_cus();
}
void set_planning_cus(int n) { g_planning_cus.store(n > 0 ? n : 0, std::memory_order_relaxed); }
int planning_cus_override() { return g_planning_cus.load(std::memory_order_relaxed); }

void launch_log_enable(bool on) { g_launch_log_on.store(on, std::memory_order_relaxed); }
void launch_log_add(const std::string& form, dim3 grid, dim3 block) {
    char buf[96];
    std::snprintf(buf, sizeof(buf), " grid=(%u,%u,%u) block=%u", grid.x, grid.y, grid.z, block.x);
    std::lock_guard<std::mutex> lk(g_log_mu);
    g_log.push_back(form + buf);
}
std::vector<std::string> launch_log_take() {
    std::lock_guard<std::mutex> lk(g_log_mu);
    std::vector<std::string> out;
    out.swap(g_log);
    return out;
}

}  // namespace dev
}  // namespace dash
