"""outeffhop_amd - MI355X (gfx950) implementation of OutEffHop's modified-softmax attention hot path.

Python host surface mirroring the reference's plugin interface:
    SOFTMAX_MAPPING, AttentionGateType, BertSelfAttentionWithExtras, OPTAttentionWithExtras,
    ViTSelfAttentionWithExtras, Association / Hopfield / HopfieldPooling, QuantizedActivation,
    Quantized{Bert,OPT}...AttentionWithExtras, QuantEmbedding / QuantizedBertEmbeddings / opt_embed_front, kurtosis / inf_norm / OutlierMeter (the reference's result metrics),
    cross_entropy / FusedCrossEntropyLoss / causal_lm_loss / masked_lm_loss / PerplexityMeter (the models' loss and the perplexity),
    dropout_add_layer_norm / FusedDropoutAddLayerNorm / FusedBertSelfOutput / FusedBertOutput / fuse_block_tails (the block tail in training),
    masked_softmax / set_fused_softmax_train (the differentiable row softmax of the unfused attention path, opt-in),
    FusedAdamW / clip_grad_norm_ (the optimizer step with the global-norm clip folded in), LossScaler (fp16 loss scaling without a host synchronisation)
over the C-ABI library `lib/liboeh_hip.so` (include/oeh.h).  There is no CPU implementation in this package:
every op raises if the HIP library is missing or a tensor is not on a GPU.
"""
from . import _lib, losses, ops, optim  # noqa: F401
from .attention import AttentionGateType, logit, set_fused_backward, set_fused_dropout, set_split_decode  # noqa: F401
from .autograd_attention import fused_attention  # noqa: F401
from .bert_attention import BertSelfAttentionWithExtras  # noqa: F401
from .layers import (FusedBertOutput, FusedBertSelfOutput, FusedDropoutAddLayerNorm, dropout_add_layer_norm, fuse_block_tails,  # noqa: F401
                     set_fused_ln_train)
from .losses import FusedCrossEntropyLoss, PerplexityMeter, causal_lm_loss, cross_entropy, masked_lm_loss  # noqa: F401
from .hopfield import Association, Hopfield, HopfieldPooling  # noqa: F401
from .opt_attention import OPTAttentionWithExtras  # noqa: F401
from .optim import FusedAdamW, LossScaler, clip_grad_norm_  # noqa: F401
from .ops import AttnFakeQuant, FakeQuantSpec, SoftmaxSpec, attn_fwd, fake_quant, inf_norm, kurtosis, outlier_stats, softmax_rows  # noqa: F401
from .outliers import OutlierMeter  # noqa: F401
from .quantization import (  # noqa: F401
    AsymmetricUniformQuantizer,
    MSE_Estimator,
    OptMethod,
    QMethods,
    QuantizationManager,
    QuantEmbedding,
    QuantizedActivation,
    QuantizedBertEmbeddings,
    QuantizedBertSelfAttentionWithExtras,
    QuantizedOPTAttentionWithExtras,
    QuantizedOPTLearnedPositionalEmbedding,
    QuantLinear,
    RangeEstimators,
    RunningMinMaxEstimator,
    get_quant_config,
    opt_embed_front,
    val_qparams,
)
from .softmax import (SOFTMAX_MAPPING, ClipSoftmax, ClipSoftmax_1, Softmax_1, clipped_softmax, clipped_softmax1, clipped_softmax_1,  # noqa: F401
                      make_clipped_softmax, make_clipped_softmax1, masked_softmax, set_fused_softmax_train, softmax_1, spec_of)
from .sparse_activations import EntmaxAlpha, Sparsemax, entmax15, entmax_bisect, sparsemax  # noqa: F401
from .vit_attention import ViTSelfAttentionWithExtras  # noqa: F401

__version__ = "0.1.0"
