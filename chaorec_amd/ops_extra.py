"""Compatibility module for the tests and tools that say `ops_extra.<name>`: it re-exports the family modules (one per
kernel file: ops_adam, ops_sparse_family, ops_dgcf, ops_vae, ops_usergraph, ops_mvgae, ops_diffmm, ops_edges, ops_mhrec, ops_bspm, ops_cfdiff, ops_wide, ops_diffrec, ops_lightgode) and
the shared helpers that once stood here, under their old names.  It defines nothing of its own -- no function, no class; new
code imports the family module or uses `chaorec_amd.ops.<name>`."""
from functools import partial

from .ops import _f32 as _vae_f32, _i32, step_tick  # noqa: F401
from .ops_adam import *  # noqa: F401,F403
from .ops_sparse_family import *  # noqa: F401,F403
from .ops_dgcf import *  # noqa: F401,F403
from .ops_vae import *  # noqa: F401,F403
from .ops_usergraph import *  # noqa: F401,F403
from .ops_mvgae import *  # noqa: F401,F403
from .ops_diffmm import *  # noqa: F401,F403
from .ops_edges import *  # noqa: F401,F403
from .ops_mhrec import *  # noqa: F401,F403
from .ops_bspm import *  # noqa: F401,F403
from .ops_cfdiff import *  # noqa: F401,F403
from .ops_wide import *  # noqa: F401,F403
from .ops_diffrec import *  # noqa: F401,F403
from .ops_lightgode import *  # noqa: F401,F403

_ug_i32 = partial(_i32, "usergraph")
