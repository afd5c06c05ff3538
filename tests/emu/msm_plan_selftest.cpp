// TEST INFRASTRUCTURE ONLY: prints what the MSM planners (csrc/msm_plan.h) decide, one line per case, on a hand-filled context and hand-filled
// base sets — no device, no library.  tests/test_emu_kernels.py feeds it the cases of tests/golden/msm_plan_cases.json and compares the lines.
//
// A case is one line of space-separated tokens:
//   msm   n=N ncols=C lane=0|1 bases=TABLES:WINDOW_BITS:LEN [knob=value ...]
//   batch n=N count=C sets=TABLES:WINDOW_BITS:LEN[;...] cols=-|i,j,... [knob=value ...]     (cols: the base set of every column; -: one set, no per-column array)
#include <stdarg.h>
#include <stdlib.h>

#include <fstream>
#include <iostream>
#include <sstream>

#include "../../halo2-lib_amd/csrc/msm_plan.h"

namespace h2 {
static char g_err[512];
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace h2
using namespace h2;

static bool set_knob(h2hip_ctx &ctx, const std::string &name, int v) {
#define KNOB_SET(knob, inherit, legal, domain) \
    if (name == #knob) {                       \
        if (!(legal)) return false;            \
        ctx.knob = v;                          \
        return true;                           \
    }
    H2_KNOB_TABLE(KNOB_SET)
#undef KNOB_SET
    return false;
}

static h2hip_bases parse_bases(const std::string &s) {
    h2hip_bases b;
    unsigned long long tables = 1, wb = 0, len = 0;
    if (sscanf(s.c_str(), "%llu:%llu:%llu", &tables, &wb, &len) != 3) {
        fprintf(stderr, "bad base set '%s'\n", s.c_str());
        exit(2);
    }
    b.tables = (uint32_t)tables;
    b.window_bits = (uint32_t)wb;
    b.n = (size_t)len;
    b.pts29 = (G1Affine *)(uintptr_t)64;   // "prepared"; never dereferenced
    return b;
}

static std::string failure(int rc) { return "rc=" + std::to_string(rc) + " err=" + g_err; }

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s CASES\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream toks(line);
        std::string kind, tok, cols = "-";
        toks >> kind;
        h2hip_ctx ctx;
        size_t n = 0, ncols = 1, count = 0;
        std::vector<h2hip_bases> sets;
        while (toks >> tok) {
            const size_t eq = tok.find('=');
            const std::string key = tok.substr(0, eq), val = tok.substr(eq + 1);
            if (key == "n") n = strtoull(val.c_str(), nullptr, 10);
            else if (key == "ncols") ncols = strtoull(val.c_str(), nullptr, 10);
            else if (key == "count") count = strtoull(val.c_str(), nullptr, 10);
            else if (key == "lane") ctx.is_lane = val == "1";
            else if (key == "cols") cols = val;
            else if (key == "bases" || key == "sets") {
                std::istringstream ss(val);
                for (std::string one; std::getline(ss, one, ';');) sets.push_back(parse_bases(one));
            } else if (!set_knob(ctx, key, atoi(val.c_str()))) {
                fprintf(stderr, "unknown token or illegal knob value '%s'\n", tok.c_str());
                return 2;
            }
        }
        g_err[0] = 0;
        std::ostringstream o;
        if (kind == "msm") {
            MsmPlan p;
            const int rc = msm_plan(ctx, sets.at(0), n, (uint32_t)ncols, &p);
            if (rc != H2HIP_OK) o << failure(rc);
            else if (p.n == 0) o << "rc=0 empty";
            else
                o << "rc=0 c=" << p.c << " Wcol=" << p.Wcol << " W=" << p.W << " B=" << p.B << " nkeys=" << p.nkeys << " emax=" << p.emax << " K1=" << p.K1
                  << " chunk=" << p.chunk << " G=" << p.G << " sort_threads=" << p.sort_threads << " hist_packed=" << p.hist_packed << " HS=" << p.HS
                  << " hist_grid=" << p.hist_grid << " hist_lds=" << p.hist_lds << " S=" << p.S << " scatter_grid=" << p.scatter_grid
                  << " scatter_lds=" << p.scatter_lds << " table_stride=" << p.table_stride << " T1=" << p.T1 << " accum_blocks=" << p.accum_blocks
                  << " len1=" << p.len1 << " blocks1=" << p.blocks1 << " bytes=" << p.digits_bytes << "," << p.bhist_bytes << "," << p.counts_bytes << ","
                  << p.offsets_bytes << "," << p.sval_bytes << "," << p.buckets_bytes << "," << p.pkey0_bytes << "," << p.pval0_bytes << "," << p.pkey1_bytes
                  << "," << p.pval1_bytes;
        } else if (kind == "batch") {
            std::vector<const h2hip_bases *> per_col;
            if (cols != "-") {
                std::istringstream ss(cols);
                for (std::string one; std::getline(ss, one, ',');) per_col.push_back(&sets.at(strtoull(one.c_str(), nullptr, 10)));
                if (per_col.size() != count) {
                    fprintf(stderr, "cols does not name %zu columns: '%s'\n", count, line.c_str());
                    return 2;
                }
            }
            BatchMsmPlan p;
            const int rc = msm_batch_plan(ctx, &sets.at(0), per_col.empty() ? nullptr : per_col.data(), n, count, H2HIP_POINT_AFFINE, &p);
            if (rc != H2HIP_OK) o << failure(rc);
            else if (p.count == 0) o << "rc=0 empty";
            else {
                o << "rc=0 NL=" << p.NL << " lane_ctxs=" << p.lane_ctxs << " fuse=" << p.fuse << " keys_per_col=" << p.keys_per_col << " deferred=" << p.deferred
                  << " buckets_bytes=" << p.buckets_bytes << " stagger=" << p.stagger << " groups=";
                for (const auto &g : p.groups) o << g.first << ":" << g.size << ":" << g.sort_waits << g.sort_signals << ",";
            }
        } else {
            fprintf(stderr, "unknown case kind '%s'\n", kind.c_str());
            return 2;
        }
        std::cout << o.str() << "\n";
    }
    return 0;
}
