"""mivod.models."""
from .llama import LlamaConfig, LlamaDecoderLayer, LlamaForCausalLM, LlamaModel  # noqa: F401
