"""graphlearn.nn.pytorch (graphlearn/python/nn/pytorch): the torch side of graphlearn.nn."""
from graphlearn.nn.pytorch.data.dataset import Dataset  # noqa: F401
from graphlearn.nn.pytorch.segment import (gat_attention, gather_rows, pair_dot, segment_aggregate,  # noqa: F401
                                            segment_softmax, weighted_segment_aggregate)
from graphlearn.nn.pytorch.layers import GATConv  # noqa: F401
from graphlearn.nn.pytorch.embedding import SparseAdagrad, SparseAdam, SparseEmbedding, SparseSGD  # noqa: F401
