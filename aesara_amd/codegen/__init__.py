"""HIP source generators, one module per kernel family.

``prelude``   the HIP text every kernel starts with, dtype tables
``scalar``    scalar programs as C++ expressions, reduction combiners, casts
``spec``      base of the kernel specs: one list of source fields gives the kernel's digest and its memo
``elemwise``  fused broadcast Elemwise / CAReduce kernels (``ew_``; LDS-tiled form ``ewt_``)
``finalize``  in-kernel finalize of full reductions, layout of the reduce workspace
``gemv_epi``  GEMV chain + Elemwise epilogue (``gv_``)
``rowpass``   single-pass row program (``rp_``)
``rowchain``  last-axis reduction chains (``rc_``, ``rcl_``)
``gemm_epi``  small-M GEMM chain + Elemwise epilogue (``ge_``)

Every spec answers ``key()`` and ``generate()`` -> (source, kernel names); nothing but the kernel
cache (``exec_common._Kernels.get``) compiles or loads what they return.
"""
from .elemwise import KernelSpec, generate, generate_tiled  # noqa: F401
from .finalize import (COLLECT_K, REDUCE_ERR_OFF, REDUCE_HOSTFLAG_OFF, TRACE_HALF, TRACE_SLOTS,  # noqa: F401
                       wave_fold_lines)
from .gemm_epi import GE_MAXDOTS, GE_MAXOPS, GemmEpiSpec, generate_gemm_epilogue  # noqa: F401
from .gemv_epi import AHIP_GV_MAXOPS, AHIP_MAXDOTS, GemvEpiSpec, generate_gemv_epilogue  # noqa: F401
from .prelude import CTYPE, PRELUDE, RTYPE  # noqa: F401
from .rowchain import (RC_MAXLEAD, RC_MAXOPS, RowChainSpec, generate_rowchain,  # noqa: F401
                       generate_rowchain_long)
from .rowpass import RP_MAXOPS, RP_MAXRED, RowPassSpec, generate_rowpass  # noqa: F401
from .scalar import (IDENTITY_SCALAR, cast, emit_scalar_body, invariant_nodes, is_float, red_combine,  # noqa: F401
                     red_identity, scalar_node_expr, store_val, sum_only_nodes)
from .spec import Spec  # noqa: F401
