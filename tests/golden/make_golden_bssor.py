"""Bit-level goldens of block SSOR on BSR storage, from the reference (oracle/_ref = Lis compiled from the reference sources by
oracle/Makefile) at T = 1 and T = 8 OpenMP threads: tests/golden/bssor_bits.npz.

  tri|<matrix>|bn<k>|w<omega>|<what>     A->WD ("wd") and lis_matrix_solve / lis_matrix_solveh with LOWER, UPPER, SSOR ("solve0" ..
                                         "solveh2", and "_alias": B is X) after lis_precon_create with -p ssor -ssor_omega <omega>
                                         -storage bsr -storage_block <k>; matrices, block sizes and omegas: tests/bssor_cases.py
  run|<matrix>|<solver>|bn<k>|T<T>|...   whole solves under bssor_cases.COMMON: "rhistory" (every bit), "x", "meta" = [iterations, status]
  model_only                             the keys the reference does not give the same bits for twice (it reads and writes x beyond n
                                         when bn does not divide n): kept out of the file, held to the model alone

The block sweeps are serial in the reference: the triangular results must not depend on T, which is asserted here before one copy is
written.  Every case is computed twice per thread count, in processes of their own, and must come out the same in every bit.
lis_precon_create runs at one thread (tests/bjacobi_cases.py, class one_thread).

    python tests/golden/make_golden_bssor.py      (needs oracle/_ref; rewrites bssor_bits.npz)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bssor_cases as cases  # noqa: E402


def main():
    runs = {}
    for T in cases.THREADS:
        tmp = os.path.join(HERE, "_bssor_T%d.npz" % T)
        runs[T] = [cases.reference_in_child(T, tmp) for _ in range(2)]
        os.unlink(tmp)
    out, model_only = {}, []
    for T in cases.THREADS:
        first, second = runs[T]
        assert sorted(first) == sorted(second)
        for k in first:
            base = k[:-len("|T%d" % T)] if k.startswith("tri|") else k
            if not cases.same_bits(first[k], second[k]):
                model_only.append(base)
            elif k.startswith("tri|"):
                if base in out:
                    assert cases.same_bits(out[base], first[k]), ("the triangular solves depend on the thread count", k)
                out[base] = first[k]
            else:
                out[k] = first[k]
    for k in set(model_only):
        out.pop(k, None)
    out["model_only"] = np.array(sorted(set(model_only)), dtype="U96")
    np.savez_compressed(os.path.join(HERE, "bssor_bits.npz"), **out)
    print(len(out) - 1, "arrays written;", len(set(model_only)), "kept on the model only:", sorted(set(model_only)))


if __name__ == "__main__":
    main()
