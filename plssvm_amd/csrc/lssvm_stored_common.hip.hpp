/*
 * lssvm_stored_common.hip.hpp -- what the sixteen-vector passes on the two 16x16x4 MFMAs share (lssvm_stored.hip, lssvm_factored.hip): the traits of the real type, sixteen
 * pointers as a kernel argument and the k-major packed vector operand.  Included INSIDE the unnamed namespace of a unit that has lssvm_types.hpp.
 */
template <typename T>
struct StoredTraits;
template <>
struct StoredTraits<float> {
    using vec = f32x4;
    using acc = f32x4;
    static constexpr int V = 4, H = 1, G = 8;  // reals per 16-byte piece, pieces per lane and block, blocks per group in flight
    __device__ static __forceinline__ int acc_row(int qd, int i) { return 4 * qd + i; }
    __device__ static __forceinline__ acc mfma(float a, float b, acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
};
template <>
struct StoredTraits<double> {
    using vec = f64x2;
    using acc = f64x4;
    static constexpr int V = 2, H = 2, G = 4;
    __device__ static __forceinline__ int acc_row(int qd, int i) { return qd + 4 * i; }
    __device__ static __forceinline__ acc mfma(double a, double b, acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
};

/* sixteen vector or result pointers as a kernel argument (selected by a chain of compares: a dynamic index would put the struct into scratch) */
template <typename T>
struct StoredVectors {
    T *p[BLOCK_VECTORS];
};
template <typename T>
__device__ __forceinline__ T *stored_select(const StoredVectors<T> &s, int u) {
    T *q = nullptr;
#pragma unroll
    for (int k = 0; k < BLOCK_VECTORS; ++k)
        if (u == k) q = s.p[k];
    return q;
}

/* Vp[column / 4][vector u][column % 4] = v_u[column] for u < count and column < n, exact zeros elsewhere: the k-major operand of both products, once per pass */
template <typename T>
__global__ __launch_bounds__(256) void k_pack_stored_v(const StoredVectors<const T> v, int count, int n, int ncols_padded, T *__restrict__ Vp) {
    const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    const size_t j = i / BLOCK_VECTORS;
    const int u = static_cast<int>(i % BLOCK_VECTORS);
    if (j >= static_cast<size_t>(ncols_padded)) return;
    const T *src = stored_select(v, u);
    Vp[((j >> 2) * BLOCK_VECTORS + u) * 4 + (j & 3)] = (u < count && j < static_cast<size_t>(n)) ? src[j] : T(0);
}
