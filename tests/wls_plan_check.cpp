// wls_plan_check.cpp — prints csrc/nct_wls_plan.h (what the S2 solver decides from the shape of its grid) as text, so that tests/test_s2_shapes.py can hold
// tests/s2_shapes.py's restatement against it: first one line with the constants, then, for every "H W" pair read from stdin, one line with every field of the
// plan, or "H W refused" with the coarsest level the solver's message names. Built with AddressSanitizer + UBSan by the test.
#include "nct_wls_plan.h"
#include <cstdio>

static void leg(const char* name, const WlsLeg& g) { printf(" %s=%dx%d:%d", name, g.tx, g.ty, g.tiles); }

int main() {
    printf("const COARSEST_N=%d MG_TAIL_N=%d MG_MAXL=%d MID_LV=%d MID_T=%d MID_MAXP0=%d MID_P1=%d MID_N1=%d mid_cap=%d,%d,%d,%d TILE_SWITCH_N=%d TXB=%d TYB=%d TYB_X0=%d TXS=%d TYS=%d LBX=%d LBY=%d\n",
           MG_COARSEST_N, MG_TAIL_N, MG_MAXL, MID_LV, MID_T, MID_MAXP0, MID_P1, MID_N1, mid_cap(1), mid_cap(2), mid_cap(3), mid_cap(4), MG_TILE_SWITCH_N, TXB, TYB, TYB_X0, TXS, TYS, LBX, LBY);
    int H, W;
    while (scanf("%d %d", &H, &W) == 2) {
        WlsPlan P;
        if (!wls_plan(H, W, P)) { printf("%d %d refused nl=%d coarsest=%d\n", H, W, P.nl, P.n[P.nl - 1]); continue; }
        printf("%d %d nl=%d levels=", H, W, P.nl);
        for (int l = 0; l < P.nl; ++l) printf("%s%dx%d:%d", l ? "," : "", P.H[l], P.W[l], P.n[l]);
        printf(" l_tail=%d tail0=%d pack_nl=%d mid_p0=%d blocks=%d", P.l_tail, P.tail0, P.pack_nl, P.mid_p0, P.blocks);
        leg("down_x0", P.down_x0);
        for (int l = 0; l < P.tail0; ++l) { printf(" big=%d", P.big[l] ? 1 : 0); leg("down", P.down[l]); leg("up", P.up[l]); }
        printf("\n");
    }
    return 0;
}
