// chain_wide_prologue.inc — what the q-split workgroup kernels of chain_wide.h do ahead of the chain: the workgroup's LDS (partial
// sums, stop word, the model's tables, q and 1/q^3 when they fit), the QTables of this wave's slice of the q-points and the
// slice's w and wI in registers.  Included verbatim, inside the kernel, so that both kernels compile from the same text.  In scope
// at the point of inclusion: M, QPL (template parameters), `const ChainArgs a`, `const double *q3inv_glb`.  It does not include
// the chain (chain_body.inc): the kernel defines the chain's hooks behind this text.
    extern __shared__ double lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NW = blockDim.x >> 6;
    const int rep = blockIdx.x;
    const int N = a.n_contrib, P = a.model.n_active, qpad = a.qpad;
    const int q0 = wave * QPL * WAVE;                              // first q index of this wave's slice
    double *part = lds, *tab = lds + WIDE_PART_DOUBLES;
    int32_t *stop_word = reinterpret_cast<int32_t *>(part + 2 * WIDE_MAX_WAVES * 4);
    // the model's tables and the per-wave row scratch (make_qtables finds the latter behind the former)
    int tabd = Contrib<M>::table_doubles(a.model.int_div);
    if constexpr (Contrib<M>::ROWTAB > 0) { if (a.model.use_rowtab) tabd += NW * Contrib<M>::ROWTAB * a.model.int_div; }
    const double *qsrc = a.q, *q3src = q3inv_glb;
    if (a.pad1) {                                                  // q and 1/q^3 fit in LDS
        double *lq = tab + tabd, *lq3 = lq + qpad;
        for (int i = tid; i < qpad; i += blockDim.x) { lq[i] = a.q[i]; lq3[i] = q3inv_glb[i]; }
        qsrc = lq; q3src = lq3;
    }
    Contrib<M>::fill_table(a.model, tab, tid, blockDim.x);
    if (tid == 0) *stop_word = 0;
    __syncthreads();
    QTables qt = make_qtables<M>(a.model, qsrc + q0, q3src + q0, tab);
    if (qt.locs_t) qt.locs_t += q0;                                // smearing: evaluation points of this slice
    double lw[QPL], lwI[QPL];
#pragma unroll
    for (int j = 0; j < QPL; ++j) { lw[j] = a.w[q0 + lane + WAVE * j]; lwI[j] = a.wI[q0 + lane + WAVE * j]; }
