"""Child process of tests/test_dia_gpu.py (not collected): the Chebyshev correction blocks on operators stored by diagonals, computed by
an engine of this process - the parent starts it with DAV_CHEB_FUSE=0, which an engine reads when it is created - and written to the npz
file named on the command line, with the apply statistics of each matrix."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import fortran_davidson_amd as fd                       # noqa: E402
from fortran_davidson_amd.engine_c import OP_A          # noqa: E402
import dia_inputs as D                                  # noqa: E402
import test_dia_gpu as T                                # noqa: E402


def main():
    out = {}
    for name, a in T.cheb_matrices().items():
        with fd.CEngine(n=a.shape[0], max_cols=66) as e:
            e.set_operator_csr(OP_A, *D.csr_of_dense(a), diagonals=True)
            e.reset_stats()
            blocks, _ = T.cheb_blocks(e, a, ms=(1, 16, 17, 33), check=False)
            st = e.stats()
        for (m, degree), t in blocks.items():
            out[f"{name}_{m}_{degree}"] = t
        out[f"{name}_applies"], out[f"{name}_cols"], out[f"{name}_bytes"] = st.applies, st.apply_cols, st.apply_bytes
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
