// Builds k_march's workgroup table on the host for the batches of tests/march_table_cfg.py and prints it whole, so that the
// Python side can apply to it the same partition check and goal predicates it applies to the table a device launch reports.
// Input (argv[1]): lines "bps channels scale a in_w m_lo m_hi frames nb cus".  Output per line:
//   TAB <line> <mode A=1 B=2> <rank-aware> <workgroups> <segs> <strips> <frames> <m_lo> <m_hi> <nb> <cus> <MS> <TAPS> <NWAVES> <TWP_OUT>
//   ENT <workgroups * segs * 4 integers: frame strip m_b m_e>
// MS, TAPS, NWAVES and TWP_OUT are MarchCfg's own.
#include <hip/hip_runtime.h>
#include <cstdio>
#include "lanczos_hip.h"
#include "lanczos_march.hpp"
using namespace lz;

template <typename T, int C, int S, int A>
static int emit(int line, int in_w, int m_lo, int m_hi, int frames, int nb, int cus) {
    using K = MarchCfg<T, C, S, A>;
    const int twp_out = K::F::TWP_OUT;
    const int strips = (in_w * S + twp_out - 1) / twp_out;   // march_issue_t
    std::vector<WgEntry> tab;
    int segs = 0;
    bool balanced = false, mode_a = false;
    const int n = march_build_table(tab, &segs, strips, frames, m_lo, m_hi, K::MS, K::TAPS, nb, cus, K::NWAVES, &balanced, &mode_a);
    if ((size_t)n * segs != tab.size()) {
        printf("BAD line %d: %d workgroups x %d segments, %zu entries\n", line, n, segs, tab.size());
        return 1;
    }
    printf("TAB %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\nENT", line, mode_a ? 1 : 2, balanced ? 1 : 0, n, segs, strips, frames, m_lo,
           m_hi, nb, cus, K::MS, K::TAPS, K::NWAVES, twp_out);
    for (const WgEntry& e : tab) printf(" %d %d %d %d", e.frame, e.tx, e.m_b, e.m_e);
    printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) {
        printf("usage: %s batches.txt\n", argv[0]);
        return 2;
    }
    int rc = 0, line = 0, bps, c, s, a, in_w, m_lo, m_hi, frames, nb, cus;
    while (fscanf(f, "%d %d %d %d %d %d %d %d %d %d", &bps, &c, &s, &a, &in_w, &m_lo, &m_hi, &frames, &nb, &cus) == 10) {
        if (bps == 1 && c == 3 && s == 2 && a == 3) rc |= emit<uint8_t, 3, 2, 3>(line, in_w, m_lo, m_hi, frames, nb, cus);
        else if (bps == 1 && c == 3 && s == 3 && a == 3) rc |= emit<uint8_t, 3, 3, 3>(line, in_w, m_lo, m_hi, frames, nb, cus);
        else if (bps == 2 && c == 4 && s == 2 && a == 4) rc |= emit<uint16_t, 4, 2, 4>(line, in_w, m_lo, m_hi, frames, nb, cus);
        else if (bps == 1 && c == 1 && s == 4 && a == 2) rc |= emit<uint8_t, 1, 4, 2>(line, in_w, m_lo, m_hi, frames, nb, cus);
        else printf("BAD line %d: no such instance here\n", line), rc = 1;
        line++;
    }
    fclose(f);
    printf(rc ? "FAILED\n" : "done %d\n", line);
    return rc;
}
