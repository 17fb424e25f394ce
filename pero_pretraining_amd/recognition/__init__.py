"""CTC fine-tuning of a pre-trained backbone into a text-line recogniser (INTEGRATION.md "From a pre-training checkpoint to a recogniser")."""
from .batch_operator import BatchOperator
from .edit_ops import EditOperations, edit_operations, top_confusions
from .lm import NGramLM
from .model import Alignment, CTCLoss, TransformerRecognizer, beam_decode, forced_align, greedy_decode, init_model
from .tester import Tester, levenshtein
from .trainer import Trainer

__all__ = ["Alignment", "BatchOperator", "CTCLoss", "EditOperations", "NGramLM", "Tester", "Trainer", "TransformerRecognizer", "beam_decode",
           "edit_operations", "forced_align", "greedy_decode", "init_model", "levenshtein", "top_confusions"]
