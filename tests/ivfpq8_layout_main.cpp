// Asks csrc/ivfpq8_layout.h from the command line (tests/test_ivfpq8_layout_cpu.py builds this with a host compiler):
//   constants  "NAME value" per constant of the layout
//   groups     stdin, "n P nlist" per line         -> "<groups_cap> <groups_fill>"
//   grid       stdin, "max_groups cus" per line    -> "<scan8_grid>"
//   lds                                            -> "scan <bytes>", "sums <bytes>", "rescore <bytes at M = 64, 1024 threads>"
//   tables     stdin, "n" per line                 -> "<tables_grid>"
//   pack       stdin, "row list sum" per line      -> "<word 0> <word 1> <list read back> <sum read back>"
#include <stdio.h>
#include <string.h>

#include "../gnn-lm_amd/csrc/ivfpq8_layout.h"

using namespace gnnlm;

// the record functions are usable in constant expressions, on the host as on the device
static_assert(surv_pack(5, 3, 2).row == 5 && surv_pack(5, 3, 2).word == (3u | 2u << 18), "the documented words");
static_assert(surv_list(surv_pack(0, (1u << SURV_LIST_BITS) - 1, SURV_SUM_BIG).word) == (1u << SURV_LIST_BITS) - 1, "list");
static_assert(surv_sum(surv_pack(0, (1u << SURV_LIST_BITS) - 1, SURV_SUM_BIG).word) == (uint32_t)SURV_SUM_BIG, "sum");

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    long long a, b, c;
    if (!strcmp(mode, "constants")) {
#define C(name) printf(#name " %d\n", (int)name);
        C(QG) C(TQ) C(QLUT_BYTES) C(TAB_BYTES) C(WAVE_CAP) C(SCAN_CTL) C(SCAN_LDS) C(HIST_BINS) C(HIST_SHIFT) C(SUMS_LDS)
        C(SURV_CNT_STRIDE) C(SURV_ROW_BITS) C(SURV_LIST_BITS) C(SURV_EXCESS_MAX) C(SURV_SUM_BIG)
        return 0;
    }
    if (!strcmp(mode, "groups")) {
        while (scanf("%lld %lld %lld", &a, &b, &c) == 3) printf("%lld %lld\n", (long long)groups_cap(a, b, c), (long long)groups_fill(groups_cap(a, b, c), c));
        return 0;
    }
    if (!strcmp(mode, "grid")) {
        while (scanf("%lld %lld", &a, &b) == 2) printf("%lld\n", (long long)scan8_grid(a, b));
        return 0;
    }
    if (!strcmp(mode, "lds")) {
        printf("scan %zu\nsums %zu\nrescore %zu\n", scan8_lds(false), scan8_lds(true), rescore_lds(64, 1024));
        return 0;
    }
    if (!strcmp(mode, "tables")) {
        while (scanf("%lld", &a) == 1) printf("%lld\n", (long long)tables_grid(a));
        return 0;
    }
    if (!strcmp(mode, "pack")) {
        while (scanf("%lld %lld %lld", &a, &b, &c) == 3) {
            const SurvRec r = surv_pack((uint32_t)a, (uint32_t)b, (uint32_t)c);
            printf("%u %u %u %u\n", r.row, r.word, surv_list(r.word), surv_sum(r.word));
        }
        return 0;
    }
    return 2;
}
