"""MI355X-native spatial meta-kriging for binary responses (drop-in for the
data-parallel core of MetaKriging_BinaryResponse.R).

The compute path is libmk.so (HIP, gfx950) behind the C ABI in include/mk.h;
this package is the host-side mirror of the reference's R interface
(spMvGLM / spPredict / partitioned_spMvGLM / the combine) over ctypes.
"""
from ._lib import MkError, load  # noqa: F401
from .session import (SamplerConfig, Session, chain_diagnostics, cholesky_batched, combine,  # noqa: F401
                      correlation_batched, correlation_cross_batched, digest, loo_compare, map_grid, psis_loo, score_grid)
from .spbayes import (load_fit, spDiag, spDiagnostics, spLoo, spMaps, spMvGLM, spPairs, spPredict, spRegions,  # noqa: F401
                      spValidate)
from .glm import glm_binomial  # noqa: F401
from .post import combine_median  # noqa: F401
from .variogram import (fit_exponential, glm_residuals, residual_variogram, suggest_phi, variogram)  # noqa: F401
from .metakriging import (combine_predictive, combine_regions, combine_results, convergence_report, meta_fit,  # noqa: F401
                          partition, partitioned_spMvGLM, posterior_summary, start_values, subset_data, validation_report)
from .node import meta_fit_node  # noqa: F401
from . import fitfile, synthetic  # noqa: F401
