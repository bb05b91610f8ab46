"""Child process of test_gmm_opt_out_paths (tests/test_kernel_edges_gpu.py).

The grouped-GEMM opt-out switches D9D_GMM_8PHASE, D9D_GMM_NN_8PHASE and
D9D_GMM_DB_8PHASE are read once per process, so the kernels behind them (the
register-staged forward/dgrad and the legacy wgrad) run at the shapes the
8-phase kernels normally take only in a process started with all three set to
0. The parent sets them; main() loops the forward and wgrad checkers of
tests/kernel_refs.py over those shapes and exits non-zero at the first
failure.
"""

import os
import sys

import torch

from tests import kernel_refs as kr

FLAGS = ("D9D_GMM_8PHASE", "D9D_GMM_NN_8PHASE", "D9D_GMM_DB_8PHASE")
DEV = "cuda"


def main():
    for flag in FLAGS:
        if os.environ.get(flag) != "0":
            print(f"{flag} is not 0: this process would test the 8-phase kernels again")
            return 2
    from d9d_amd.ops._ext import get_ext

    ext = get_ext()

    def fwd(op):
        return lambda a, w, bs: op(a.to(DEV), w.to(DEV), bs)

    def db(a, g, bs, E):
        return ext.gmm_db(a.to(DEV), g.to(DEV), bs, E)

    done = 0
    try:
        for sizes in kr.GMM_ROW_LAYOUTS:
            for K, N in kr.GMM_NT_8PHASE + kr.GMM_BOTH_8PHASE:
                kr.check_gmm_fwd(fwd(ext.gmm_nt), "nt", sizes, K, N)
                done += 1
            for K, N in kr.GMM_BOTH_8PHASE:
                kr.check_gmm_fwd(fwd(ext.gmm), "nn", sizes, K, N)
                done += 1
        for sizes in (kr.GMM_ROWS_EDGE, kr.GMM_ROWS_EMPTY, kr.GMM_ROWS_CHUNKS):
            for K, N in kr.GMM_DB_8PHASE:
                kr.check_gmm_db(db, sizes, K, N)
                done += 1
        kr.check_gmm_db(db, kr.GMM_POISON_ROWS, 192, 256, poison_expert=1)
        torch.cuda.synchronize()
    except AssertionError as exc:
        print(f"failed after {done} cases: {exc}")
        return 1
    print(f"{done + 1} fallback cases passed")
    return 0


if __name__ == "__main__":
    sys.exit(main())
