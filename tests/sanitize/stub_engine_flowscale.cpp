// TEST INFRASTRUCTURE ONLY - never linked into a product library.
// The flow-scale entry points of include/rife_hip.h for the sanitizer builds of the host side: what csrc/rife.cpp calls from RIFE::set_flow_scale, i.e. what
// `rife-hip -d 2` sends.  The stub engine of stub_engine.cpp blends its inputs whatever the divisor is, so this file only keeps the value per engine and
// answers the argument rules of the real call (before load, not a power of two, 4 and above); the family rules are the CLI's own, by directory name.
#include <map>
#include <mutex>

#include "../../include/rife_hip.h"

struct rife_hip { bool loaded = false; int gpuid = 0; };      // the definition of stub_engine.cpp, token for token

static std::mutex g_flowscale_mu;
static std::map<const rife_hip*, int> g_flowscale;      // engines that left the default; an address reused by a later engine starts from its own set call

extern "C" {

int rife_hip_set_flow_scale(rife_hip_t* r, int divisor) {
    if (!r || !r->loaded) return -RIFE_HIP_EINVAL;
    if (divisor <= 0 || (divisor & (divisor - 1))) return -RIFE_HIP_EINVAL;
    if (divisor > 2) return -RIFE_HIP_ENOSYS;
    std::lock_guard<std::mutex> g(g_flowscale_mu);
    g_flowscale[r] = divisor;
    return 0;
}

int rife_hip_flow_scale(const rife_hip_t* r) {
    std::lock_guard<std::mutex> g(g_flowscale_mu);
    const auto it = g_flowscale.find(r);
    return it == g_flowscale.end() ? 1 : it->second;
}

}
