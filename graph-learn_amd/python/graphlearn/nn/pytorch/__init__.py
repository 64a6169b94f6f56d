"""graphlearn.nn.pytorch (graphlearn/python/nn/pytorch): the torch side of graphlearn.nn."""
from graphlearn.nn.pytorch.data.dataset import Dataset  # noqa: F401
from graphlearn.nn.pytorch.segment import (dot_attention, gat_attention, gather_rows, pair_dot,  # noqa: F401
                                            segment_aggregate, segment_softmax, weighted_segment_aggregate)
from graphlearn.nn.pytorch.layers import GATConv, TransformerConv  # noqa: F401
from graphlearn.nn.pytorch.embedding import SparseAdagrad, SparseAdam, SparseEmbedding, SparseSGD  # noqa: F401
from graphlearn.nn.pytorch.memory import TGNMemory, TimeEncoder  # noqa: F401
