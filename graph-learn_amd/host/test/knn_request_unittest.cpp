// Host-only behaviour of KnnRequest / KnnResponse (contrib/knn/knn_request.cc): the reference's tensor and
// parameter names, Clone, Partition to every shard, and Stitch under the search's total order.  No device.
#include <cmath>
#include <cstring>
#include <vector>

#include "glx.h"
#include "graphlearn/graphlearn.h"
#include "test_util.h"

using namespace graphlearn;  // NOLINT

TEST(KnnRequestTest, FieldsCloneAndFactory) {
  KnnRequest req("item", 5);
  const float in[6] = {1, 2, 3, 4, 5, 6};
  req.Set(in, 2, 3);
  EXPECT_EQ(req.Name(), std::string("KnnOperator"));
  EXPECT_EQ(req.Type(), std::string("item"));
  EXPECT_EQ(req.K(), 5);
  EXPECT_EQ(req.BatchSize(), 2);
  EXPECT_EQ(req.Dimension(), 3);
  // the reference's names: knn_request.cc:58-69,113-122
  EXPECT_EQ(req.params_.at(kType).GetString(0), std::string("item"));
  EXPECT_EQ(req.params_.at(kSideInfo).Size(), 3);
  EXPECT_EQ(req.tensors_.at(kFloatAttrKey).Size(), 6);
  for (int i = 0; i < 6; ++i) EXPECT_EQ(req.Inputs()[i], in[i]);
  OpRequest* c = req.Clone();
  KnnRequest* ck = static_cast<KnnRequest*>(c);
  EXPECT_TRUE(ck->K() == 5 && ck->BatchSize() == 2 && ck->Dimension() == 3 && ck->Inputs()[5] == 6.0f);
  delete c;
  OpRequest* fr = RequestFactory::GetInstance()->NewRequest("KnnOperator");
  OpResponse* fs = RequestFactory::GetInstance()->NewResponse("KnnOperator");
  EXPECT_TRUE(dynamic_cast<KnnRequest*>(fr) != nullptr && dynamic_cast<KnnResponse*>(fs) != nullptr);
  delete fr;
  delete fs;
  EXPECT_TRUE(op::OpFactory::GetInstance()->Create("KnnOperator") != nullptr);
}

TEST(KnnRequestTest, PartitionSendsTheRequestToEveryShard) {
  SetGlobalFlagServerCount(3);
  KnnRequest req("item", 2);
  const float in[2] = {1, 2};
  req.Set(in, 1, 2);
  ShardsPtr<OpRequest> shards = req.Partition(1);
  EXPECT_EQ(shards->Size(), 3);
  EXPECT_TRUE(shards->Get(1) == &req);
  for (int i = 0; i < 3; ++i) {
    KnnRequest* p = static_cast<KnnRequest*>(shards->Get(i));
    EXPECT_TRUE(p != nullptr && !p->IsShardable());
    EXPECT_TRUE(p->K() == 2 && p->BatchSize() == 1 && p->Dimension() == 2 && p->Inputs()[1] == 2.0f);
  }
  EXPECT_TRUE(shards->Get(0) != &req && shards->Get(0) == shards->Get(2));
  SetGlobalFlagServerCount(1);
}

static KnnResponse* Part(int32_t batch, int32_t k, const std::vector<int64_t>& ids, const std::vector<float>& dist) {
  KnnResponse* r = new KnnResponse;
  r->Init(batch, k);
  std::memcpy(r->MutableIds(), ids.data(), ids.size() * sizeof(int64_t));
  std::memcpy(r->MutableDistances(), dist.data(), dist.size() * sizeof(float));
  return r;
}

TEST(KnnRequestTest, StitchMergesUnderTheTotalOrder) {
  const float nan = std::nanf(""), inf = INFINITY;
  // one query, k = 4, three shards; ties (2.0 in shards 0 and 1; +0 and -0), a NaN, padding
  for (int metric = 0; metric < 2; ++metric) {
    SetGlobalFlagKnnMetric(metric);
    const float pad = metric == 1 ? -inf : inf;
    const float s = metric == 1 ? -1.0f : 1.0f;  // IP: larger is better, so mirror the values
    ShardsPtr<OpResponse> shards(new Shards<OpResponse>(3));
    shards->Add(0, Part(1, 4, {10, 11, 12, 13}, {s * -0.0f, s * 2.0f, s * 2.0f, nan}), true);
    shards->Add(1, Part(1, 4, {20, 21, -1, -1}, {s * 0.0f, s * 2.0f, pad, pad}), true);
    shards->Add(2, Part(1, 4, {30, 31, 32, -1}, {s * 1.0f, s * 5.0f, nan, pad}), true);
    KnnResponse out;
    out.Stitch(shards);
    EXPECT_TRUE(out.BatchSize() == 1 && out.K() == 4);
    const int64_t want[4] = {10, 20, 30, 11};  // zeros tie: lower shard first; then 1; then the first 2.0 of shard 0
    for (int j = 0; j < 4; ++j) EXPECT_EQ(out.Ids()[j], want[j]);
    EXPECT_TRUE(std::signbit(out.Distances()[0]) != std::signbit(out.Distances()[1]));  // the bits are carried
    EXPECT_EQ(out.params_.at(kSideInfo).Size(), 2);
    EXPECT_TRUE(out.tensors_.count(kNodeIds) == 1 && out.tensors_.count(kDistances) == 1);
  }
  // fewer entries than k: numbers, then NaNs by (shard, position), then padding
  SetGlobalFlagKnnMetric(0);
  ShardsPtr<OpResponse> shards(new Shards<OpResponse>(2));
  shards->Add(0, Part(1, 3, {1, 2, -1}, {nan, nan, inf}), true);
  shards->Add(1, Part(1, 3, {3, -1, -1}, {7.0f, inf, inf}), true);
  KnnResponse out;
  out.Stitch(shards);
  EXPECT_TRUE(out.Ids()[0] == 3 && out.Ids()[1] == 1 && out.Ids()[2] == 2);
  // one shard: its response as it is
  ShardsPtr<OpResponse> one(new Shards<OpResponse>(1));
  one->Add(0, Part(2, 1, {5, 6}, {1.0f, 2.0f}), true);
  KnnResponse single;
  single.Stitch(one);
  EXPECT_TRUE(single.BatchSize() == 2 && single.K() == 1 && single.Ids()[1] == 6);
}

int main() { return RunAllTests(); }
