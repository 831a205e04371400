// CsrMatrix of include/ark_hip.hpp (mul, mul_t, bilinear) driven from a compiled C++ program on the GPU over BLS12-381 Fr,
// against vectors the caller computed with big integers:
//   argv: dir name...   for every name, dir holds <name>_dims.bin (rows, cols, nnz as u64), <name>_row_ptr.bin and
//                       <name>_col_idx.bin (u32), <name>_vals.bin, <name>_x.bin (cols elements), <name>_u.bin (rows elements),
//                       <name>_y.bin (M x), <name>_yt.bin (M^T u) and <name>_b.bin (u^T M x, one element); elements are 4
//                       little-endian u64 limbs
// Built and run by tests/test_gpu_cpp_csr.py (g++, links libark_hip.so).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "ark_hip.hpp"
using namespace ark_hip;

static int fails = 0;
#define EXPECT(c, msg) do { if (!(c)) { std::printf("FAIL: %s: %s\n", name.c_str(), msg); fails++; } } while (0)

constexpr int FIELD = ARK_HIP_BLS12_381_FR;
using V = DeviceVec<FIELD>;

template <class T>
static std::vector<T> read(const std::string& path, size_t count) {
  std::vector<T> v(count);
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f || std::fread(v.data(), sizeof(T), count, f) != count) { std::printf("cannot read %s\n", path.c_str()); std::exit(3); }
  std::fclose(f);
  return v;
}

int main(int argc, char** argv) {
  static_assert(sizeof(Fr) == 32, "an element is four u64 limbs");
  if (ark_hip_device_count() <= 0) { std::printf("no GPU\n"); return 2; }
  if (argc < 3) { std::printf("usage: csr_check dir name...\n"); return 3; }
  const std::string dir = std::string(argv[1]) + "/";
  size_t long_rows_seen = 0, stream_only_seen = 0;
  for (int k = 2; k < argc; k++) {
    const std::string name = argv[k], at = dir + name + "_";
    const std::vector<uint64_t> dims = read<uint64_t>(at + "dims.bin", 3);
    const size_t rows = dims[0], cols = dims[1], nnz = dims[2];
    const std::vector<uint32_t> row_ptr = read<uint32_t>(at + "row_ptr.bin", rows + 1), col_idx = read<uint32_t>(at + "col_idx.bin", nnz);
    const std::vector<Fr> vals = read<Fr>(at + "vals.bin", nnz), x = read<Fr>(at + "x.bin", cols), u = read<Fr>(at + "u.bin", rows);
    const std::vector<Fr> y = read<Fr>(at + "y.bin", rows), yt = read<Fr>(at + "yt.bin", cols), b = read<Fr>(at + "b.bin", 1);
    const CsrPlan p = csr_plan(rows, row_ptr.data());
    EXPECT(p.tile > 0 && p.blocks + p.long_rows > 0, "the plan");
    (p.long_rows ? long_rows_seen : stream_only_seen)++;

    CsrMatrix<FIELD> m(rows, cols, row_ptr, col_idx, vals, true);
    EXPECT(m.rows() == rows && m.cols() == cols && m.nnz() == nnz && m.has_transpose(), "the dimensions");
    V dx = V::from_vec(x), du = V::from_vec(u);
    EXPECT(m.mul(dx).to_vec() == y, "mul");
    EXPECT(m.mul_t(du).to_vec() == yt, "mul_t");
    EXPECT(m.bilinear(du, dx) == b[0], "bilinear");
    V out = V::from_vec(u);   // garbage of the right length: overwritten in full
    m.mul(dx, out);
    EXPECT(out.to_vec() == y, "mul into a given vector");
    EXPECT(dx.to_vec() == x && du.to_vec() == u, "inputs untouched");
    {
      CsrMatrix<FIELD> plain(rows, cols, row_ptr, col_idx, vals);
      EXPECT(plain.mul(dx).to_vec() == y, "mul without the transpose");
      bool threw = false;
      try { plain.mul_t(du); } catch (const Error&) { threw = true; }
      EXPECT(threw, "mul_t refuses a handle without the transpose");
    }
    {
      bool threw = false;
      try { m.mul(V(cols + 1)); } catch (const Error&) { threw = true; }
      EXPECT(threw, "mul refuses a vector of the wrong length");
      threw = false;
      std::vector<uint32_t> bad = col_idx;
      if (nnz) bad[nnz / 2] = (uint32_t)cols;
      try { CsrMatrix<FIELD> w(rows, cols, row_ptr, bad, vals); } catch (const Error&) { threw = true; }
      EXPECT(threw || !nnz, "create refuses a column index equal to cols");
    }
  }
  const std::string name = "all";
  EXPECT(long_rows_seen > 0 && stream_only_seen > 0, "the caller chose one stream-block matrix and one long-row matrix");
  if (fails) return 1;
  std::printf("all ok\n");
  return 0;
}
