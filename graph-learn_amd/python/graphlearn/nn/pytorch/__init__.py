"""graphlearn.nn.pytorch (graphlearn/python/nn/pytorch): the torch side of graphlearn.nn."""
from graphlearn.nn.pytorch.data.dataset import Dataset  # noqa: F401
from graphlearn.nn.pytorch.segment import (gather_rows, pair_dot, segment_aggregate, segment_softmax,  # noqa: F401
                                            weighted_segment_aggregate)
from graphlearn.nn.pytorch.embedding import SparseAdagrad, SparseAdam, SparseEmbedding, SparseSGD  # noqa: F401
