// Asks csrc/star_route.h from the command line (tests/test_star_chain_ref_cpu.py builds this with a host compiler):
//   route      stdin, one shape per line: T H kg M dsub D  (M > 0: the PQ source, D = M * dsub; M = 0: dense rows of D floats)
//              -> "<route name> <staged 0 / 1> <dynamic LDS bytes> <threads> <heads per pass>"; the switch comes from the
//              environment as in the library
//   constants  "NAME value" per constant of the dispatch
#include <stdio.h>
#include <string.h>

#include "../gnn-lm_amd/csrc/star_route.h"

using namespace gnnlm;

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    if (!strcmp(mode, "constants")) {
#define C(name) printf(#name " %d\n", (int)name);
        C(HB) C(KGM) C(CD) C(TPW) C(TABF) C(SCS) C(STAR_THREADS) C(STAR_TAB_THREADS) C(STAR_LDS_MAX) C(STAR_LDS_TWO_WG)
        return 0;
    }
    if (strcmp(mode, "route")) return 2;
    static float row[4];
    static uint8_t code[16];
    long long T, H, kg, M, dsub, D;
    while (scanf("%lld %lld %lld %lld %lld %lld", &T, &H, &kg, &M, &dsub, &D) == 6) {
        gnnlm_star_attn_t p = {};
        p.T = (int32_t)T; p.H = (int32_t)H; p.kg = (int32_t)kg; p.D = (int32_t)D;
        if (M > 0) { p.codes = code; p.centroids = row; p.M = (int32_t)M; p.dsub = (int32_t)dsub; }
        else { p.X = row; p.ldx = D; p.x_group_stride = 1; }
        const StarPlan plan = star_route(p, star_switches());
        printf("%s %d %zu %d %d\n", star_route_name(plan.route), (int)plan.staged, plan.lds_bytes, plan.threads, plan.heads_per_pass);
    }
    return 0;
}
