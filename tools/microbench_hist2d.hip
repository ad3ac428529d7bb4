// microbench_hist2d.hip — device time of hist2d_kernel alone (mcsas_amd/csrc/hist2d_kernel.h: what mcsas_hip_histogram2d launches),
// by HIP events around single launches: one histogram of nx x ny cells over N contributions and R repetitions, uniform values that
// all lie inside the edges.  The ownership walk costs N iterations per wave whatever the cell count; 0 x 0 runs the moments alone.
// Prints one JSON line per shape: median, min and max of the timed launches in microseconds.  Build (tools/hist2d_cost.py does it):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -I mcsas_amd/csrc tools/microbench_hist2d.hip -o tools/microbench_hist2d
// Run: tools/microbench_hist2d [N R repeats]   (default 4096 50 21)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hist2d_kernel.h"

#define CHK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

int main(int argc, char **argv) {
    const int N = argc > 1 ? atoi(argv[1]) : 4096, R = argc > 2 ? atoi(argv[2]) : 50, repeats = argc > 3 ? atoi(argv[3]) : 21, P = 2;
    if (N < 1 || N > HIST2D_MAX_CONTRIBS || R < 1 || repeats < 1) { printf("N 1..%d, R >= 1, repeats >= 1\n", HIST2D_MAX_CONTRIBS); return 1; }
    const int shapes[][2] = {{0, 0}, {1, 1}, {8, 8}, {32, 32}, {64, 64}};
    srand(1);
    std::vector<double> c((size_t)N * P * R), f((size_t)8 * N * R);
    for (double &v : c) v = (rand() + 0.5) / ((double)RAND_MAX + 1.);          // inside (0, 1)
    for (double &v : f) v = (rand() + 0.5) / ((double)RAND_MAX + 1.) / N;
    double *dc, *df, *de, *dout;
    Hist2dSpecDev *ds;
    CHK(hipMalloc(&dc, sizeof(double) * c.size())); CHK(hipMalloc(&df, sizeof(double) * f.size()));
    CHK(hipMalloc(&de, sizeof(double) * 2 * (HIST2D_MAX_CELLS + 2))); CHK(hipMalloc(&ds, sizeof(Hist2dSpecDev)));
    CHK(hipMalloc(&dout, sizeof(double) * ((size_t)2 * HIST2D_MAX_CELLS * R + 7 * R)));
    CHK(hipMemcpy(dc, c.data(), sizeof(double) * c.size(), hipMemcpyHostToDevice));
    CHK(hipMemcpy(df, f.data(), sizeof(double) * f.size(), hipMemcpyHostToDevice));
    hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    for (const auto &sh : shapes) {
        const int nx = sh[0], ny = sh[1];
        std::vector<double> edges;
        for (int k = 0; k <= nx; ++k) edges.push_back(nx ? (double)k / nx : 0.);
        for (int k = 0; k <= ny; ++k) edges.push_back(ny ? (double)k / ny : 0.);
        const Hist2dSpecDev s{0, 1, 0, nx, ny, 0, 0, 0, 0., 1., 0., 1.};
        CHK(hipMemcpy(de, edges.data(), sizeof(double) * edges.size(), hipMemcpyHostToDevice));
        CHK(hipMemcpy(ds, &s, sizeof s, hipMemcpyHostToDevice));
        const size_t lds = hist2d_staged_bytes(N) + hist2d_shared_bytes(N, nx, ny);
        if (lds > 64 * 1024) CHK(hipFuncSetAttribute((const void *)hist2d_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        std::vector<float> us;
        for (int i = 0; i < repeats + 3; ++i) {                               // (three warm-up launches)
            CHK(hipEventRecord(e0, nullptr));
            hist2d_kernel<<<(unsigned)R, WAVE, lds>>>(N, P, R, dc, df, de, ds, dout);
            CHK(hipGetLastError());
            CHK(hipEventRecord(e1, nullptr));
            CHK(hipEventSynchronize(e1));
            float ms; CHK(hipEventElapsedTime(&ms, e0, e1));
            if (i >= 3) us.push_back(ms * 1e3f);
        }
        std::vector<double> back((size_t)2 * nx * ny * R + 7 * R);
        CHK(hipMemcpy(back.data(), dout, sizeof(double) * back.size(), hipMemcpyDeviceToHost));
        double in_cells = 0.;
        for (size_t k = 0; k < (size_t)nx * ny; ++k) in_cells += back[k * R];
        std::sort(us.begin(), us.end());
        printf("{\"nx\": %d, \"ny\": %d, \"N\": %d, \"R\": %d, \"lds_bytes\": %zu, \"launches\": %zu, \"median_us\": %.2f, \"min_us\": %.2f, \"max_us\": %.2f, "
               "\"cells_sum_rep0\": %.6f, \"total_rep0\": %.6f}\n", nx, ny, N, R, lds, us.size(), us[us.size() / 2], us.front(), us.back(), in_cells,
               back[(size_t)2 * nx * ny * R]);
    }
    return 0;
}
