"""dagnn_amd - MI355X-native (gfx950) implementation of DAGNN's layer-by-layer message-passing path.

Drop-in modules with the reference's constructor / state_dict / forward(G) contracts:

    from dagnn_amd import DAGNN, ASTNodeEncoder        # ogbg-code/model/dagnn.py, ogbg-code/utils.py
    from dagnn_amd import DAGNN_NA, DAGNN_BN           # dvae/dagnn.py (DAGNN), dvae/dagnn_bn.py
    from dagnn_amd import DataParallel                 # ogbg-code/tg/data_parallel.py (list[Batch] caller)
    from dagnn_amd import evaluate, SeqF1              # ogbg-code/main_pyg.py:91-124 (predicted tokens, the F1 evaluator)
    from dagnn_amd import ASTNodeEncoder2, lp          # ogbg-code/utils2.py, ogbg-code/main_pyg_lp.py (the LP task)
    from dagnn_amd import GraphStore                   # the loader side: the dataset on the device, a batch per launch
    from dagnn_amd import EpochMeter, seq_ce_step      # ogbg-code/main_pyg.py:39-88 (train(): loss, tokens, train metric per launch)
    from dagnn_amd import DagStore                     # the same for D-VAE data sets (ENAS / BN rows), dvae/train.py's loops
    from dagnn_amd import attach_predictor             # dvae/train.py --predictor: the MLP on mu, its MSE and gradients
    from dagnn_amd import BnData, bn_scores            # bayesian_optimization/evaluate_BN.py: BIC scores of BN structures
    from dagnn_amd import SparseGP, bo_round           # bayesian_optimization/sparse_gp.py: the model that proposes BO points

The hot path runs in libdagnn_hip.so (hand-written HIP, C ABI in include/dagnn_hip.h); importing
this package does not need a GPU, calling `forward` does.
"""
from .constants import *  # noqa: F401,F403
from .data import (GraphBatch, GraphData, augment_edge2, collate_sharded, collate_with_plan,  # noqa: F401
                   shard_by_nodes)
from .host_plan import attach_plan, build_plan_host  # noqa: F401
from .dvae import DAGNN_BN, DAGNN_NA  # noqa: F401
from .model import DAGNN, ASTNodeEncoder, ASTNodeEncoder2  # noqa: F401
from .train import EpochMeter, GradBucket, seq_ce_step  # noqa: F401
from . import evaluate  # noqa: F401
from .evaluate import SeqF1, SeqLoss  # noqa: F401
from .attention import Attention, attention_host  # noqa: F401   (model.attention(G): per-edge attention weights of a pass)
from . import lp  # noqa: F401
from .lp import ClassAccuracy, class_ce_step, class_cross_entropy, evaluate_lp, lp_batches, lp_targets  # noqa: F401
from .data_parallel import DataParallel  # noqa: F401
from .store import GraphStore  # noqa: F401
from .dvae_store import DagStore  # noqa: F401
from . import predictor  # noqa: F401
from .predictor import attach_predictor, predict_latent, predictor_mse, predictor_report  # noqa: F401
from . import bn_score  # noqa: F401
from .bn_score import BnData, BnEvaluator, bn_scores, decode_and_score, score_dense, score_strings, store_scores  # noqa: F401
from . import sgp  # noqa: F401
from .sgp import SparseGP, bo_round  # noqa: F401

__version__ = "0.1.0"
