// TEST INFRASTRUCTURE ONLY - never linked into a product library.
// The precision entry points of include/rife_hip.h for the sanitizer builds of the host side: what csrc/rife.cpp calls from RIFE::set_precision, i.e. what
// `rife-hip -p fast` sends.  The stub engine of stub_engine.cpp blends its inputs whatever the precision is, so this file only keeps the value per engine and
// answers the argument rules of the real call (before load, a value that is neither constant); the family and mode rules are the CLI's own.
#include <map>
#include <mutex>

#include "../../include/rife_hip.h"

struct rife_hip { bool loaded = false; int gpuid = 0; };      // the definition of stub_engine.cpp, token for token

static std::mutex g_precision_mu;
static std::map<const rife_hip*, int> g_precision;      // engines that left the default; an address reused by a later engine starts from its own set call

extern "C" {

int rife_hip_set_precision(rife_hip_t* r, int precision) {
    if (!r || !r->loaded) return -RIFE_HIP_EINVAL;
    if (precision != RIFE_HIP_PRECISION_FULL && precision != RIFE_HIP_PRECISION_FAST) return -RIFE_HIP_EINVAL;
    std::lock_guard<std::mutex> g(g_precision_mu);
    g_precision[r] = precision;
    return 0;
}

int rife_hip_precision(const rife_hip_t* r) {
    std::lock_guard<std::mutex> g(g_precision_mu);
    const auto it = g_precision.find(r);
    return it == g_precision.end() ? RIFE_HIP_PRECISION_FULL : it->second;
}

}
