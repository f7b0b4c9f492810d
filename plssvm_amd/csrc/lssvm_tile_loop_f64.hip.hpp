/*
 * lssvm_tile_loop_f64.hip.hpp -- the 128 x 128 tile loop on v_mfma_f64_16x16x4_f64 that the kernels of the fixed-size model (lssvm_reduced.hip: k_reduced_gram,
 * k_reduced_leverage, k_reduced_leverage_prefix, k_landmark_product, k_cross_product) and the assembly of the stored kernel matrix (lssvm_stored.hip: k_store_gram) share.
 * Included inside the unnamed namespace of the unit that uses it.
 *
 * A workgroup of 256 threads forms one 128 x 128 tile of A B^T; its four waves hold 64 x 64 each (wave = 2 wr + wc: row half wr, column half wc) as sixteen accumulators.
 * Both operands go through LDS in steps of RG_KC = 16 of the contraction index.  Lane 16 qd + r of a wave reads, per MFMA, entry (row r of a 16-row block, index qd of the
 * k-step) of either operand and holds rows qd + 4 i, column r of each 16 x 16 block of the result.  A row-major operand (RG_LS doubles between two rows) is staged by
 * thread -> (row srow [+ 32 p], indices 2 sseg, 2 sseg + 1 of the step): eight threads load the 16 indices of a row as one line.
 */
struct TileLanes {
    int tid, lane, wave, wr, wc, r, qd, srow, sseg;
    __device__ __forceinline__ TileLanes() :
        tid(threadIdx.x), lane(tid & 63), wave(tid >> 6), wr(wave >> 1), wc(wave & 1), r(lane & 15), qd(lane >> 4), srow(tid >> 3), sseg(tid & 7) {}
};

/* the sixteen accumulators of a wave, zeroed */
__device__ __forceinline__ void tile_zero(f64x4 (&acc)[4][4]) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            acc[mt][nt] = f64x4{ 0.0, 0.0, 0.0, 0.0 };
            // the start values live in the accumulators' OWN registers (C == D for every MFMA of a chain): lssvm_tile_f64_wide.hip.hpp has the hazard this keeps away
            asm volatile("" : "+v"(acc[mt][nt]));
        }
}

/* acc += A B^T over `nsteps` steps.  stage_load(s) takes step s from memory into registers, stage_store() puts them into LDS: the loads of step s + 1 are in flight under
 * the 64 MFMAs of step s (whatever is done to the staged values belongs into stage_store: the step's MFMAs stand between a load and its first use).  Ab / Bb: the lane's
 * first entry of either operand in LDS; A's block t, k-sub-step ks is Ab[t A_T + ks A_KS], B's is Bb[t 16 RG_LS + 4 ks].  Every accumulator is one chain over s and ks
 * ascending.  Ends behind a barrier: every wave has read the last step. */
template <int A_T, int A_KS, typename Load, typename Store>
__device__ __forceinline__ void tile_contract(int nsteps, const double *Ab, const double *Bb, f64x4 (&acc)[4][4], Load stage_load, Store stage_store) {
    if (nsteps > 0) {
        stage_load(0);
        stage_store();
    }
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const bool has_next = s + 1 < nsteps;
        if (has_next) stage_load(s + 1);
#pragma unroll
        for (int ks = 0; ks < RG_KC / 4; ++ks) {
            double av[4], bv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                av[t] = Ab[t * A_T + ks * A_KS];
                bv[t] = Bb[t * 16 * RG_LS + ks * 4];
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
        }
        __syncthreads();  // (every wave has read this step)
        if (has_next) {
            stage_store();
            __syncthreads();
        }
    }
}
