// KnnRequest / KnnResponse and the "KnnOperator" (graphlearn/src/contrib/knn/knn_request.cc, knn_op.cc:29-59): the
// search itself is one C-ABI call on the node type's device table (glx_knn_search) -- the table IS the flat index.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "glx.h"
#include "graphlearn/config.h"
#include "graphlearn/graph_store.h"
#include "graphlearn/knn_request.h"
#include "graphlearn/operator.h"

namespace graphlearn {

namespace {
const char* const kKnnOpName = "KnnOperator";

// GLOBAL_FLAG(KnnMetric) as the C-ABI's metric: the values are the reference's (config.cc:107, flat_index.cc:27-28)
int KnnMetricOfFlag() { return GLOBAL_FLAG(KnnMetric) == 1 ? GLX_KNN_IP : GLX_KNN_L2; }

// the order-preserving image of a distance that glx_knn.hip uses: ascending = better first, +0 == -0, NaN last
uint32_t OrderImage(float d, int metric) {
  uint32_t bits;
  std::memcpy(&bits, &d, sizeof(bits));
  if ((bits & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if (bits == 0x80000000u) bits = 0;
  const uint32_t asc = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  return metric == GLX_KNN_L2 ? asc : ~asc;
}
}  // namespace

KnnRequest::KnnRequest() : OpRequest(), clone_(nullptr) {
  ADD_TENSOR(params_, kOpName, kString, 1);
  params_[kOpName].AddString(kKnnOpName);
}

KnnRequest::KnnRequest(const std::string& type, int32_t k) : OpRequest(), clone_(nullptr) {
  ADD_TENSOR(params_, kOpName, kString, 1);
  params_[kOpName].AddString(kKnnOpName);
  ADD_TENSOR(params_, kType, kString, 1);
  params_[kType].AddString(type);
  ADD_TENSOR(params_, kSideInfo, kInt32, 3);
  params_[kSideInfo].AddInt32(k);
}

KnnRequest::~KnnRequest() { delete clone_; }

OpRequest* KnnRequest::Clone() const {
  KnnRequest* req = new KnnRequest(Type(), K());
  req->Set(Inputs(), BatchSize(), Dimension());
  return req;
}

ShardsPtr<OpRequest> KnnRequest::Partition(int32_t own_shard) const {
  OpRequest* self = const_cast<KnnRequest*>(this);
  self->DisableShard();
  if (clone_ == nullptr) {
    clone_ = Clone();
    clone_->DisableShard();
  }
  const int32_t n = GLOBAL_FLAG(ServerCount) < 1 ? 1 : GLOBAL_FLAG(ServerCount);
  ShardsPtr<OpRequest> ret(new Shards<OpRequest>(n));
  for (int32_t i = 0; i < n; ++i) ret->Add(i, i == own_shard ? self : clone_, false);
  return ret;
}

void KnnRequest::Set(const float* inputs, int32_t batch_size, int32_t dimension) {
  params_[kSideInfo].AddInt32(batch_size);
  params_[kSideInfo].AddInt32(dimension);
  ADD_TENSOR(tensors_, kFloatAttrKey, kFloat, batch_size * dimension);
  tensors_[kFloatAttrKey].AddFloat(inputs, inputs + (size_t)batch_size * dimension);
}

const std::string& KnnRequest::Type() const { return params_.at(kType).GetString(0); }
int32_t KnnRequest::K() const { return params_.at(kSideInfo).GetInt32(0); }
int32_t KnnRequest::BatchSize() const { return params_.at(kSideInfo).GetInt32(1); }
int32_t KnnRequest::Dimension() const { return params_.at(kSideInfo).GetInt32(2); }
const float* KnnRequest::Inputs() const { return tensors_.at(kFloatAttrKey).GetFloat(); }

KnnResponse::KnnResponse() : OpResponse() {}

void KnnResponse::Init(int32_t batch_size, int32_t k) {
  batch_size_ = batch_size;
  ADD_TENSOR(params_, kSideInfo, kInt32, 2);
  params_[kSideInfo].AddInt32(batch_size);
  params_[kSideInfo].AddInt32(k);
  ADD_TENSOR(tensors_, kNodeIds, kInt64, batch_size * k);
  tensors_[kNodeIds].Resize(batch_size * k);
  ADD_TENSOR(tensors_, kDistances, kFloat, batch_size * k);
  tensors_[kDistances].Resize(batch_size * k);
}

int32_t KnnResponse::BatchSize() const { return params_.at(kSideInfo).GetInt32(0); }
int32_t KnnResponse::K() const { return params_.at(kSideInfo).GetInt32(1); }
const int64_t* KnnResponse::Ids() const { return tensors_.at(kNodeIds).GetInt64(); }
const float* KnnResponse::Distances() const { return tensors_.at(kDistances).GetFloat(); }
int64_t* KnnResponse::MutableIds() { return tensors_[kNodeIds].MutableInt64(); }
float* KnnResponse::MutableDistances() { return tensors_[kDistances].MutableFloat(); }

void KnnResponse::Stitch(ShardsPtr<OpResponse> shards) {
  std::vector<KnnResponse*> parts;
  int32_t shard_id = 0;
  OpResponse* tmp = nullptr;
  shards->ResetNext();
  while (shards->Next(&shard_id, &tmp)) parts.push_back(static_cast<KnnResponse*>(tmp));
  if (parts.empty()) return;
  if (parts.size() == 1) {
    OpResponse::Swap(*parts[0]);
    return;
  }
  const int32_t batch = parts[0]->BatchSize(), k = parts[0]->K();
  const int metric = KnnMetricOfFlag();
  Init(batch, k);
  int64_t* ids = MutableIds();
  float* dist = MutableDistances();
  struct Entry {
    uint64_t key;  // image of the distance, then part * k + position
    int64_t id;
    float dist;
  };
  std::vector<Entry> all;
  for (int32_t q = 0; q < batch; ++q) {
    all.clear();
    for (size_t p = 0; p < parts.size(); ++p) {
      const int64_t* pi = parts[p]->Ids() + (size_t)q * k;
      const float* pd = parts[p]->Distances() + (size_t)q * k;
      for (int32_t j = 0; j < k; ++j) {
        if (pi[j] == -1) continue;  // padding: absent
        all.push_back(Entry{((uint64_t)OrderImage(pd[j], metric) << 32) | (uint32_t)(p * k + j), pi[j], pd[j]});
      }
    }
    std::sort(all.begin(), all.end(), [](const Entry& a, const Entry& b) { return a.key < b.key; });
    for (int32_t j = 0; j < k; ++j) {
      const bool have = (size_t)j < all.size();
      ids[(size_t)q * k + j] = have ? all[j].id : -1;
      dist[(size_t)q * k + j] = have ? all[j].dist : (metric == GLX_KNN_L2 ? INFINITY : -INFINITY);
    }
  }
}

REGISTER_REQUEST(KnnOperator, KnnRequest, KnnResponse)

namespace op {

class KnnOperator : public Operator {
public:
  Status Process(const OpRequest* req, OpResponse* res) override {
    const KnnRequest* request = static_cast<const KnnRequest*>(req);
    KnnResponse* response = static_cast<KnnResponse*>(res);
    if (!graph_store_) return error::InvalidArgument("operator is not bound to a GraphStore");
    // the index of a type is a property of the store's own Noder: another store's type of the same name has its own
    Noder* noder = graph_store_->GetNoder(request->Type());
    if (!noder->KnnIndexed() || noder->Device() == nullptr) {
      return error::InvalidArgument("Invalid node type.");  // knn_op.cc:33-38
    }
    if (request->Dimension() != noder->GetSideInfo()->f_num) {
      return error::InvalidArgument("KNN inputs have " + std::to_string(request->Dimension()) + " columns, node type '" +
                                    request->Type() + "' has " + std::to_string(noder->GetSideInfo()->f_num));
    }
    const int32_t n = request->BatchSize(), k = request->K();
    response->Init(n, k);
    int rc = glx_knn_search(noder->Device(), KnnMetricOfFlag(), request->Inputs(), n, k, response->MutableIds(),
                            response->MutableDistances(), GLX_PTR_HOST, nullptr);
    return error::FromGlx(rc);
  }
};

REGISTER_OPERATOR("KnnOperator", KnnOperator);

}  // namespace op
}  // namespace graphlearn
