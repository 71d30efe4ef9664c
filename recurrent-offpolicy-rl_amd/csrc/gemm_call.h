// Host side of the GEMM family (gemm_f32.hip, gemm_bf3.hip, gemm_any.hip, gemm_bf16.hip): one description of a product, what the
// matrix-core kernels can read, the operand-layout dispatch, and the functions the four files call in each other.  No device code.
#pragma once
#include "resel_common.h"
#include <type_traits>

namespace resel {

// C[b] = epi(A[b] (.) B[b] + bias[b]) as an extern "C" entry receives it: the entry fills one of these, every layer below reads it.
// Leading dimensions and batch strides in elements; an operand is [rows][K] (kcontig) or [K][rows].
struct GemmCall {
    const void* A; int64_t lda, strideA; int a_kcontig;          // fp32; bf16 only in the rows form of resel_gemm_bf16
    const float* B; int64_t ldb, strideB; int b_kcontig;
    const float* bias; int64_t strideBias; int act;              // act: 0 none, 1 ELU, 2 C += product, 3 softplus; gemm_bf3_launch: 4 / 5 with GemmFused
    void* C; int64_t ldc, strideC; void* workspace;               // C: fp32; bf16 when gemm_any_launch is told OUT_BF16
    int M, N, K, batch;
    const float *amax_a, *amax_b;                                 // magnitude handles of A and B (product mode 2), else nullptr
    unsigned long long* amax_c; unsigned amax_epoch;              // optional: where the epilogue publishes max |C|
    hipStream_t s;
};
// operands of the third edition's fused epilogues (act 4: Y and the column-sum partials; act 5: w3 and the row dots)
struct GemmFused { const float* aux = nullptr; int64_t ldaux = 0, strideAux = 0; float* red = nullptr; int redrows = 0; };
// The 32-bit piece offsets of the matrix-core kernels span 128 rows or 32 k of the leading dimension (a 24-bit multiply in the third
// edition): row strides of 2^22 elements and more belong to gemm_any.hip.  The only place that knows the bound.
inline bool gemm_ld_in_reach(int64_t lda, int64_t ldb) { return lda < ((int64_t)1 << 22) && ldb < ((int64_t)1 << 22); }
// What the matrix-core kernels can read: four consecutive elements along each operand's contiguous axis per load - 16-byte (bf16
// operand: 8-byte) aligned bases, leading dimensions, batch strides and the contiguous extents multiples of 4 - and row strides in reach.
inline bool gemm_mfma_readable(const GemmCall& c, bool a_bf16 = false, bool b_bf16 = false) {
    const auto aligned = [](const void* p, bool bf16) { return !(reinterpret_cast<uintptr_t>(p) & (bf16 ? 7u : 15u)); };
    return c.lda % 4 == 0 && c.ldb % 4 == 0 && c.strideA % 4 == 0 && c.strideB % 4 == 0 && aligned(c.A, a_bf16) && aligned(c.B, b_bf16) &&
           (c.a_kcontig ? c.K : c.M) % 4 == 0 && (c.b_kcontig ? c.K : c.N) % 4 == 0 && gemm_ld_in_reach(c.lda, c.ldb);
}
// The run-time operand layouts as template arguments: f(std::bool_constant<a_kcontig>, std::bool_constant<b_kcontig>).
template <typename F>
inline auto with_layout(int a_kcontig, int b_kcontig, F&& f) {
    if (a_kcontig) return b_kcontig ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
    return b_kcontig ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}
// gemm_bf3.hip: the split modes on 256 x 128 tiles (second edition; third edition for mode 2 with whole K steps, which also has the
// fused epilogues).  split in {2, 3, 6}, K >= 32, M > 128; argument checks are the caller's.
size_t gemm_bf3_workspace_bytes(int M, int N, int K, int batch);
bool gemm_bf3_fused_ok(int M, int N, int K);
int gemm_bf3_launch(const GemmCall& c, int split, const GemmFused& fused = {});
// gemm_any.hip: the shapes the matrix-core editions do not take (unaligned rows, tiny reductions) and the M <= 8 rollout rows; argument
// checks are the caller's.  rnd: A, B (and the bias), the fp32 result rounded to bf16; C stored as bf16; A is bf16 (rows form only)
constexpr int RND_A = 1, RND_B = 2, RND_OUT = 4, OUT_BF16 = 8, A_BF16 = 16;
size_t gemm_any_workspace_bytes(int M, int N, int K, int batch);
bool gemm_any_rows_ok(const GemmCall& c, bool a_bf16 = false);
int gemm_any_launch(const GemmCall& c, int rnd);

}  // namespace resel
