// Host build of csrc/vprog.h for tests/test_native_vprog.py (a shared object called through ctypes).
#include <cstring>

#include "vprog.h"

using namespace zk;

extern "C" {

// shape = (n_wires, n_slots, n_consts, n_constraints, n_rows, S).  Writes the error text (empty:
// the program is accepted), the COMMIT rows as (row, wire) pairs (room for n_rows of them) and
// has_emul; returns the number of COMMIT rows.
int vprog_check(const uint32_t* shape, const uint32_t* prog, uint32_t* commit, int* has_emul,
                char* err, size_t err_len) {
  std::vector<std::pair<uint32_t, uint32_t>> rows;
  bool emul = false;
  const std::string e = vprog_validate(
      VprogShape{shape[0], shape[1], shape[2], shape[3], shape[4], shape[5]}, prog, &rows, &emul);
  std::strncpy(err, e.c_str(), err_len - 1);
  err[err_len - 1] = 0;
  for (size_t i = 0; i < rows.size(); i++) {
    commit[2 * i] = rows[i].first;
    commit[2 * i + 1] = rows[i].second;
  }
  *has_emul = emul;
  return (int)rows.size();
}

// the 26 opcodes and the 12 classes in the order of tests/test_native_vprog.py's name lists
void vprog_constants(uint32_t* ops, uint32_t* cls) {
  const uint32_t o[26] = {OP_END, OP_ADD, OP_SUB, OP_MUL, OP_MULC, OP_ADDC, OP_NEG, OP_INV, OP_BITS,
                          OP_SETC, OP_ABC, OP_COPY, OP_DIV, OP_BATCHINV, OP_PAIR, OP_MULABC,
                          OP_XORABC, OP_XOR, OP_FMAC, OP_FMA, OP_HIST, OP_HQ, OP_COMMIT, OP_BXOR,
                          OP_BAND, OP_EMUL};
  const uint32_t c[12] = {CLS_M, CLS_X, CLS_A, CLS_R, CLS_I, CLS_BITS, CLS_BINV, CLS_HIST,
                          CLS_COMMIT, CLS_B_SCHED, CLS_EMUL, CLS_LIMBS};
  std::memcpy(ops, o, sizeof o);
  std::memcpy(cls, c, sizeof c);
}

}
