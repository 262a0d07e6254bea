// Optional per-dispatch timing (bench.py), the implementation of what sr_profile.h declares: start/stop events ride on the dispatch
// packet itself (isr_launch), so no extra barrier packets or cache flushes perturb the stream.  Every translation unit of the library
// records through isr_profile_record; the records are read back through isrProfile* (include/isr_sr_kernels.h).
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/isr_sr_kernels.h"
#include "sr_profile.h"

struct ProfileRecord { int variant; double flops; hipEvent_t e0, e1; };
static bool g_profile = false;
static bool g_profile_small = false;      // isrProfileEnable(2): also the frame's small kernels (variants >= ISR_VARIANT_TRUNK_PACK)
static std::vector<ProfileRecord> g_records;
static std::vector<hipEvent_t> g_event_pool;
static size_t g_pool_used = 0;
static hipEvent_t pool_event()
{
    if (g_pool_used == g_event_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        g_event_pool.push_back(e);
    }
    return g_event_pool[g_pool_used++];
}

void isr_profile_record(int variant, double flops, hipEvent_t* e0, hipEvent_t* e1)
{
    if (!g_profile || (isr_variant_is_small(variant) && !g_profile_small)) return;
    *e0 = pool_event(); *e1 = pool_event();
    g_records.push_back({ variant, flops, *e0, *e1 });
}

extern "C" {

int isrProfileEnable(int on)
{
    g_profile = on != 0;
    g_profile_small = on == 2;
    g_records.clear();
    g_pool_used = 0;
    return 0;
}

int isrProfileCount(void) { return (int)g_records.size(); }

int isrProfileGet(int i, int* variant, double* flops, float* ms)
{
    if (i < 0 || i >= (int)g_records.size()) return -1;
    const ProfileRecord& r = g_records[i];
    float t = 0.f;
    if (!r.e0 || !r.e1 || hipEventElapsedTime(&t, r.e0, r.e1) != hipSuccess) return -2;
    *variant = r.variant; *flops = r.flops; *ms = t;
    return 0;
}

}  // extern "C"
