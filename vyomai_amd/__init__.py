"""vyomai_amd -- MI355X-native implementation of VyomAI's transformer hot path.

Same public names as the reference package (VyomAI/__init__.py:1-12) for everything on that
path; the math runs in hand-written gfx950 HIP kernels behind the C ABI in include/vyom_hip.h.
"""
from .utils import EncoderConfig  # noqa: F401
from .layers.kv_cache import DynamicCache, StaticCache, StaticCacheOne, DynamicCacheOne  # noqa: F401
from .models.encoder import EncoderModel, EncoderForMaskedLM, EncoderForSequenceClassification  # noqa: F401
from .models.decoder import DecoderModel  # noqa: F401
from .models.electra import Discriminator, ElectraModel, ElectraLoss  # noqa: F401
from . import pretraining  # noqa: F401
from .models.vision_encoder import Vit  # noqa: F401
from .models.multimodel import VisionLanguageModel  # noqa: F401
from .models.encoder_decoder import EncoderDecoderModel  # noqa: F401
from .models.custom_transformer import (Config, MLP, Attention, RMSNorm, DecoderLayer, BaseModel,  # noqa: F401
                                         ModelForCausalLM)
from .models import qwen3  # noqa: F401
from .models.qwen3 import Qwen3Model, load_weights_into_qwen  # noqa: F401
from .serving import RadixNode, SequenceState, PagedKVManager, ContinuousBatchEngine, SamplingParams  # noqa: F401
from .adapters import LoraAdapters, LoraLinear, add_lora, disable_lora, lora_state_dict, merge_lora  # noqa: F401
from .adapters import DoraLinear, add_dora, disable_dora, dora_state_dict, merge_dora  # noqa: F401
from .generation_utils import generate, generate_multimodel, generate_seq2seq  # noqa: F401
from .logits_processors import (LogitsProcessor, GreedyProcessor, MultinomialProcessor, TopKProcessor,  # noqa: F401
                                NucleusProcessor, TopKNucleusProcessor)
from .speculative_decoding import speculative_generate  # noqa: F401
