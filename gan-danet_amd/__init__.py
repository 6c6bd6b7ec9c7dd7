"""gan_danet_amd -- MI355X-native (gfx950) implementation of the GAN-DANet G+D training hot path.

Host side: PyTorch-ROCm for device memory, streams, the autograd tape and ``torch.distributed`` (RCCL).
Arithmetic: hand-written HIP kernels in ``csrc/`` behind the C ABI of ``include/gandanet.h``
(``lib/libgandanet_hip.so``).  There is no CPU path: without the built library, or on CPU tensors, the
modules raise.

The directory is called ``gan-danet_amd`` (repo contract); import it as ``gan_danet_amd`` -- the
repo-root ``gan_danet_amd.py`` registers the package under that name -- or through the reference's own
import paths ``from models import ...`` / ``from model import ...``.
"""
from .config import config, layer_override, precision, set_precision, set_sync_bn
from .kern import set_deterministic, set_split_reduce
from .attention import attention_report, cam_attention, pam_attention_rows, pam_attention_stats
from .discriminator import SRGAND, Discriminator1
from . import filters
from . import spline
from . import prepare
from . import basins
from . import stl
from .stl import detrend_and_compare, stl_decompose
from . import timeseries
from .timeseries import SeriesSkill, coarsen, consistency, harmonic_fit, lstsq_series, skill_maps, taylor_stats
from . import trend
from .trend import TrendTest, mann_kendall, normal_quantile, sen_slope, trend_test
from . import changepoint
from .changepoint import ChangePoint, ChangePoints, change_point, change_points, cusum, pettitt, segmented_fit
from .evaluate import RegressionMetrics, evaluate, evaluate_ensemble
from . import verification
from .verification import EnsembleVerification, ensemble_scores
from . import eof
from .eof import EOFResult, eof_analysis
from . import spectra
from .spectra import (CrossSpectrum, Spectrum, cross_spectrum, effective_resolution, power_spectrum,
                      spectral_ratio)
from . import drought
from .drought import (DSI_CLASSES, DroughtClimatology, DroughtEvents, climatology, compare_events, drought_area, drought_events,
                      drought_index)
from . import clusters
from .clusters import DroughtClusters, drought_clusters, label_components, structure_word
from . import neighborhood
from .neighborhood import FSSResult, drought_fss, fractions_skill_score, fss_cross_grid, neighborhood_fraction
from . import biascorrect
from .biascorrect import QuantileMap, series_quantiles
from . import lagcorr
from .lagcorr import (LagCorrelation, autocorrelation, correlation_significance, driver_lags, fdr_threshold,
                      lag_correlation)
from . import collocation
from .collocation import (TripleCollocation, TripleCollocationBootstrap, bootstrap_indices, triple_collocation,
                          triple_collocation_bootstrap)
from . import ssa
from .ssa import SSAFill, SSAResult, ssa_decompose, ssa_fill
from . import regions
from .regions import Regions, kmeans_scan, kmeans_series, region_agreement
from .generator import (CAMModule, CBAMBlock, DANetAttention, DenseBlock, DenseLayer, FlexibleUpsamplingModule,
                        OriginalRelationshipLearner, PAMModule, SqueezeExcitation, TransitionLayer)
from .losses import SSIM, BCEWithLogitsLoss, MSELoss, PerceptualLoss, TVLoss
from .optim import AdamW
from .train import GanTrainer
from .utils import weights_init_normal

__all__ = [
    "CBAMBlock", "FlexibleUpsamplingModule", "OriginalRelationshipLearner", "SqueezeExcitation",
    "Discriminator1", "SRGAND", "PerceptualLoss", "SSIM", "TVLoss", "weights_init_normal",
]
