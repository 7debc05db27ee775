// Host-side record of the convolution-family launches: which instantiation each layer problem ran (see afan_common.h).
// Off by default; tests switch it on around a call or an iteration and read the records back to tell which kernel variant
// served which problem.  No device work and no synchronisation: records are taken when the launch is enqueued.
#include "afan_common.h"
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <vector>

namespace afan {
namespace trace {

struct Problem {
    int op;
    int64_t n, hi, wi, ci, co;
    int k, stride, dilation;
};
struct Rec {
    Problem p;
    char name[64];
};

int g_on = 0;
static std::mutex g_mu;
static std::vector<Rec> g_recs;
static thread_local Problem t_cur[4];
static thread_local int t_count = 0;

void problem(int slot, int op, int64_t n, int64_t hi, int64_t wi, int64_t ci, int64_t co, int k, int stride, int dilation) {
    if (slot < 0 || slot >= 4) return;
    t_cur[slot] = Problem{op, n, hi, wi, ci, co, k, stride, dilation};
    t_count = slot + 1;
}

int op() { return t_count > 0 ? t_cur[0].op : -1; }

void launch(const char* fmt, ...) {
    Rec r;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(r.name, sizeof(r.name), fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lk(g_mu);
    if (t_count == 0) {                       // a launch whose entry point named no problem: recorded as such (op -1)
        r.p = Problem{-1, 0, 0, 0, 0, 0, 0, 0, 0};
        g_recs.push_back(r);
    }
    for (int i = 0; i < t_count; ++i) {
        r.p = t_cur[i];
        g_recs.push_back(r);
    }
    t_count = 0;                              // one launch per named call: a later launch must name its own problem
}

}  // namespace trace
}  // namespace afan

extern "C" {

int afan_conv_trace(int on) {
    std::lock_guard<std::mutex> lk(afan::trace::g_mu);
    if (on) afan::trace::g_recs.clear();
    __atomic_store_n(&afan::trace::g_on, on ? 1 : 0, __ATOMIC_RELAXED);
    return AFAN_OK;
}

int afan_conv_trace_read(int64_t* problems, char* names, int max_records) {
    using namespace afan::trace;
    std::lock_guard<std::mutex> lk(g_mu);
    const int total = (int)g_recs.size();
    if (max_records > 0 && (!problems || !names)) return AFAN_ENULL;
    for (int i = 0; i < total && i < max_records; ++i) {
        const Problem& p = g_recs[i].p;
        int64_t* o = problems + 9 * (int64_t)i;
        o[0] = p.op; o[1] = p.n; o[2] = p.hi; o[3] = p.wi; o[4] = p.ci; o[5] = p.co; o[6] = p.k; o[7] = p.stride; o[8] = p.dilation;
        snprintf(names + 64 * (int64_t)i, 64, "%s", g_recs[i].name);
    }
    return total;
}

}  // extern "C"
