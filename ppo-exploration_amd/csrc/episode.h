// Per-env episode bookkeeping shared by the device environments (env.hip, env_real.hip):
// the running return / length, and the SB3 Monitor-style record of the episode that ended
// at this step (NaN / 0 when none did).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace ppox {

struct Episode {
    float* ep_ret;
    int32_t* ep_len;
    float* done_ret;  // nullable: return of the episode that ended at this step, NaN otherwise
    int32_t* done_len;
};

__device__ inline void episode_update(const Episode& ep, long long n, float rew, bool done) {
    if (!ep.ep_ret) return;
    const float r = ep.ep_ret[n] + rew;
    const int l = ep.ep_len[n] + 1;
    if (ep.done_ret) ep.done_ret[n] = done ? r : __builtin_nanf("");
    if (ep.done_len) ep.done_len[n] = done ? l : 0;
    ep.ep_ret[n] = done ? 0.f : r;
    ep.ep_len[n] = done ? 0 : l;
}

}  // namespace ppox
