// Lock-free union-find, shared by the connected-component labellers (lws_speckle.hip: the pixels of a disparity map; lws_objects.hip:
// the cells of a u-disparity image): one tile in LDS, then the tile-local roots across workgroups in global memory.
// The invariant every loop rests on: parent[i] <= i in the index order of the caller, always (a root is the FIRST element of its
// set, a union hangs the later root under the earlier one with an atomic min).  A find walk therefore strictly decreases and ends
// after at most i steps whatever other workgroups do meanwhile; no loop waits for another thread's progress.
#pragma once
#include "lws_common.h"

namespace lws::cclkit {

// ---- union-find in LDS (one tile) ----
// par[i] <= i: the walk strictly decreases, so it ends.
__device__ __forceinline__ int lds_find(const volatile int *par, int i)
{
    for (int n = par[i]; n != i; n = par[i]) i = n;
    return i;
}

// Every round ends the call or strictly lowers max(a, b) (the atomic min hangs the later root a under the earlier one b; when
// another thread re-parented a first, its old parent `o` < a takes a's place and the union goes on as (o, b)), so the loop ends.
__device__ __forceinline__ void lds_unite(int *par, int a, int b)
{
    for (;;) {
        a = lds_find(par, a);
        b = lds_find(par, b);
        if (a == b) return;
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        const int o = atomicMin(&par[a], b);
        if (o == a) return;
        a = o;
    }
}

// ---- union-find in global memory across workgroups: agent-scope atomics only ----
__device__ __forceinline__ int ld_agent(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// par[i] <= i, and a parent only ever decreases: the walk strictly decreases, so it ends (after at most i steps).
__device__ __forceinline__ int g_find(const int *par, int i)
{
    for (int n = ld_agent(par + i); n != i; n = ld_agent(par + i)) i = n;
    return i;
}

// As lds_unite: every round returns or strictly lowers max(a, b); it never waits for another workgroup.
__device__ __forceinline__ void g_unite(int *par, int a, int b)
{
    for (;;) {
        a = g_find(par, a);
        b = g_find(par, b);
        if (a == b) return;
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        const int o = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (o == a) return;
        a = o;                                              // a had been hung under o < a meanwhile: o and b are still to be joined
    }
}

}  // namespace lws::cclkit
