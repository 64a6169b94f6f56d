// KnnRequest / KnnResponse with the reference's surface and its tensor / parameter names
// (graphlearn/src/contrib/knn/knn_request.h, knn_request.cc:58-69,113-122,147-157).
#ifndef GLX_HOST_KNN_REQUEST_H_
#define GLX_HOST_KNN_REQUEST_H_
#include <string>

#include "graphlearn/op_request.h"
#include "graphlearn/partition.h"

namespace graphlearn {

// Request: [batch_size, dimension] query vectors for the node type's table.  params: kOpName = "KnnOperator",
// kType = the node type, kSideInfo = {k, batch_size, dimension}; tensors: kFloatAttrKey = the vectors.
class KnnRequest : public OpRequest {
public:
  KnnRequest();
  KnnRequest(const std::string& type, int32_t k);
  ~KnnRequest() override;

  OpRequest* Clone() const override;
  // knn_request.cc:93-111: every server searches its own rows, so the whole request goes to every shard
  // (this object itself to shard `own_shard`, one shared clone to the others; the shards own neither).
  ShardsPtr<OpRequest> Partition(int32_t own_shard = 0) const;
  void Set(const float* inputs, int32_t batch_size, int32_t dimension);

  const std::string& Type() const;
  int32_t K() const;
  int32_t BatchSize() const;
  int32_t Dimension() const;
  const float* Inputs() const;

private:
  mutable OpRequest* clone_;
};

// Response: ids and distances, [batch_size, k] each.  params: kSideInfo = {batch_size, k}; tensors: kNodeIds, kDistances.
class KnnResponse : public OpResponse {
public:
  KnnResponse();
  OpResponse* New() const override { return new KnnResponse; }

  void Init(int32_t batch_size, int32_t k);
  int32_t BatchSize() const;
  int32_t K() const;
  const int64_t* Ids() const;
  const float* Distances() const;
  int64_t* MutableIds();
  float* MutableDistances();

  // knn_request.cc:159-202: one shard's response is taken as it is; several are merged per query under the total
  // order of the search (include/glx.h, glx_knn_merge): a better distance under GLOBAL_FLAG(KnnMetric) first, then the
  // lower shard, then the earlier position; a NaN distance after every number; id -1 (padding) last.  The reference's
  // heap leaves the order of equal distances to chance.
  void Stitch(ShardsPtr<OpResponse> shards);
};

}  // namespace graphlearn
#endif  // GLX_HOST_KNN_REQUEST_H_
