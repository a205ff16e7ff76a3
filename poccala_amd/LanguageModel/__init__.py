"""The language-model package the reference's decoder imports (Decoder.py:17) and does not ship."""
from .Ngram import Ngram  # noqa: F401
