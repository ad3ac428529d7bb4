// pipe_geometry_check.hip — the producer side of pipe_geometry (csrc/pipe_layout.h) as a stand-alone host program:
// tests/test_pipe_geometry_host.py compiles and runs it.  No GPU: pipe_layout.h holds no device code.
//   pipe_geometry_check nq n_contrib n_chains   one line: rc kb w rows_per_wave prod_blocks_y sub_per_block gram_lds lazy_rows
//                                               gram_off drow_off rec_off prod_lds — a model without a table or an integral
//                                               (the sphere) on a 256-CU device, nothing asked for by a tuning word
#include <cstdio>
#include <cstdlib>

#include "pipe_layout.h"

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    mcsas::PipeGeom g{};
    const int rc = mcsas::pipe_geometry(atoi(argv[1]), atoi(argv[2]), 0, 0, 0, 0, 0, 0, atoi(argv[3]), 256, &g, 4);
    printf("%d %d %d %d %d %d %d %d %d %d %d %llu\n", rc, g.kb, g.w, g.rows_per_wave, g.prod_blocks_y, g.sub_per_block, g.gram_lds, g.lazy_rows,
           g.gram_off, g.drow_off, g.rec_off, (unsigned long long)g.prod_lds);
    return 0;
}
