from .config import GPTConfig, OptimizerConfig, PRESETS
from .gpt import GPT, Block, CausalSelfAttention, MLP
from .generation import generate, generate_batch, generate_beam, generate_speculative, quantize_int8_, score

__all__ = ["GPTConfig", "OptimizerConfig", "PRESETS", "GPT", "Block", "CausalSelfAttention", "MLP", "generate",
           "generate_batch", "generate_beam", "generate_speculative", "quantize_int8_", "score"]
