from .qwen3 import Qwen3Model, load_weights_into_qwen  # noqa: F401
