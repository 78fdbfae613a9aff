"""Pre-training collators with the reference's names (VyomAI/pretraining)."""
from .collators import (LanguageModeling, electra, log, masked_language_modeling, noise, sample)  # noqa: F401
