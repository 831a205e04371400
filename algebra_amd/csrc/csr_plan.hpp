// How the rows of a CSR matrix are cut into work for the kernels of spmv.cuh.  Pure host code, no HIP:
// ark_hip_fr_csr_create builds a handle's descriptors with it and ark_hip_csr_plan reports its counts, so tests pin the rule
// without a GPU (the arrangement of msm_plan.hpp and ark_hip_prefix_scan_plan).
//
// The rule, one pass over row_ptr:
//   * a row with more than CSR_TILE nonzeros is a LONG row: it closes the open stream block, stands alone and is cut into
//     ceil(nnz / CSR_TILE) chunks of CSR_TILE nonzeros (the last one ragged);
//   * any other row joins the open STREAM block unless the block would then hold more than CSR_TILE nonzeros or already holds
//     CSR_MAX_ROWS rows (empty rows count); then the block is closed and the row opens the next one.
// So the blocks cover the rows exactly once and in order, a stream block never exceeds CSR_TILE nonzeros or CSR_MAX_ROWS
// rows, and the sum of the chunks is sum ceil(nnz / CSR_TILE) over the long rows.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace arkhip {

constexpr int CSR_TILE = 2048;       // nonzeros per workgroup: the limb planes of polyops.cuh hold one product each
constexpr int CSR_MAX_ROWS = 2048;   // rows per stream block: a lane adds at most 8 rows
static_assert(CSR_TILE <= (1 << 16), "the header promises a tile of at most 2^16 nonzeros");

struct CsrPlan {
  std::vector<uint32_t> stream;   // per stream block: first row, one past its last row
  std::vector<uint32_t> chunk;    // per chunk of a long row: the row, the chunk's index inside it
  std::vector<uint32_t> lrow;     // per long row: the row, its first partial, its number of chunks
  size_t stream_blocks() const { return stream.size() / 2; }
  size_t long_chunks() const { return chunk.size() / 2; }
  size_t long_rows() const { return lrow.size() / 3; }
};

// row_ptr: rows + 1 non-decreasing entries (validated by the caller); keep == false only counts
inline void csr_plan_rows(size_t rows, const uint32_t* row_ptr, bool keep, CsrPlan* out, size_t* n_stream, size_t* n_long,
                          size_t* n_chunks) {
  size_t ns = 0, nl = 0, nc = 0;
  size_t open = 0;             // first row of the open block
  size_t open_rows = 0, open_nnz = 0;
  auto close = [&](size_t end) {
    if (open_rows) {
      if (keep) { out->stream.push_back((uint32_t)open); out->stream.push_back((uint32_t)end); }
      ns++;
    }
    open_rows = 0;
    open_nnz = 0;
  };
  for (size_t r = 0; r < rows; r++) {
    const size_t len = (size_t)row_ptr[r + 1] - row_ptr[r];
    if (len > (size_t)CSR_TILE) {
      close(r);
      const size_t k = (len + CSR_TILE - 1) / CSR_TILE;
      if (keep) {
        out->lrow.push_back((uint32_t)r); out->lrow.push_back((uint32_t)nc); out->lrow.push_back((uint32_t)k);
        for (size_t j = 0; j < k; j++) { out->chunk.push_back((uint32_t)r); out->chunk.push_back((uint32_t)j); }
      }
      nl++;
      nc += k;
      continue;
    }
    if (open_rows && (open_nnz + len > (size_t)CSR_TILE || open_rows == (size_t)CSR_MAX_ROWS)) close(r);
    if (!open_rows) open = r;
    open_rows++;
    open_nnz += len;
  }
  close(rows);
  if (n_stream) *n_stream = ns;
  if (n_long) *n_long = nl;
  if (n_chunks) *n_chunks = nc;
}

}  // namespace arkhip
