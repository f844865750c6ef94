// Interfaces of check.hip used by amdzk_check_witness (prover.hip): the kernels that TEST a witness instead of storing
// anything — failing gates, lookup inputs outside their table, copy constraints between unequal cells.
#pragma once
#include "plonk_kernels.hpp"

// One more instruction of Lagrange-domain programs, executed by expr_check_kernel only: pop the top of stack; where it is
// a non-zero residue on a row < usable, constraint `arg` has one more failing row. (Beside plonk_kernels.hpp's ExprOp,
// whose interpreters ignore it.)
constexpr uint32_t OP_CHECK = 24;

// What a check leaves per constraint: count[c] failing rows, the smallest of them in first[c] (UINT32_MAX: none). The
// caller clears both before the kernels run (count to 0, first to 0xFF bytes).
struct CheckCounters {
  unsigned long long* count;
  uint32_t* first;
};

// A Lagrange-domain program (ExprArgs as for zk_expr_eval, radix 2^256) whose values end in OP_CHECK instead of OP_STORE.
int zk_check_expr(amdzk_ctx* ctx, const ExprArgs& a, uint32_t depth, uint32_t usable, CheckCounters out, const char* name);
// inputs / tables: [L][n] canonical keys (Fr::to_repr), every table sorted ascending with its rows >= usable padded by
// all-ones keys (zk_sort_keys' convention): input row r < usable of lookup l fails constraint first_constraint + l when
// its key is none of the table's first `usable` keys.
int zk_check_lookups(amdzk_ctx* ctx, const bn254::Fr* d_inputs, const bn254::Fr* d_tables, size_t L, uint32_t n, uint32_t usable,
                     uint32_t first_constraint, CheckCounters out);
// sigma: [S][n] Montgomery values delta^i' omega^j' -> cells[c * n + j] = (i', j'). d_tab: S values delta^(i * 2^k), S values
// delta^(-i), k values omega^(-(2^b)). A value that is no delta^i omega^j with i < S leaves (c << 32 | j) + 1 of the smallest
// such cell in *d_bad (the caller sets it to all ones: none).
int zk_sigma_decode(amdzk_ctx* ctx, const bn254::Fr* d_sigma, uint32_t S, uint32_t k, const bn254::Fr* d_tab, uint2* d_cells,
                    unsigned long long* d_bad);
// cell (c, j) of the permutation fails constraint first_constraint + c when its value differs from the value of the cell
// d_cells names for it; d_cols[c]: the Lagrange values of permutation column c (n rows).
int zk_check_copies(amdzk_ctx* ctx, const bn254::Fr* const* d_cols, const uint2* d_cells, uint32_t S, uint32_t n, uint32_t first_constraint,
                    CheckCounters out);
