// bpsw_chain_tables_core.h -- the per-read arithmetic of chain_tables_kernel (bpsw_chain_dev.hip): from the pools the chain stage
// filled slice by slice to the tables chain2aln_kernel indexes (ChainBatchDev, bpsw_internal.h), in read order.
//
// __host__ __device__: the kernel calls chain_tables_read one read per lane, and tests/chain_tables_host/chain_tables_host.cpp
// compiles the same function with g++ against the arrays bpsw_chain2aln_batch's host loop builds from the same chains.
//
// The pools: pool_cnt holds the seed count of every kept chain and pool_seeds the seeds of those chains, a read's chains next to
// each other in the read's own chain order, the reads in the order the slices (and the calling thread's reads) wrote them.
// where[r] says where read r's part begins in both and how long it is.  The caller has scanned the (chains, seeds) columns of
// `where` in read order: chain_at / seed_at are the chains and the seeds in kept chains of the reads before r.
#pragma once
#include <stdint.h>

#include "bpsw.h"

#if defined(__HIPCC__)
#define BPSW_TABLES_HD __host__ __device__ __forceinline__
#else
#define BPSW_TABLES_HD inline
#endif

namespace bpsw {

struct ChainWhere {  // 24 bytes
  long long cnt_at, seed_at;  // the read's first entry of pool_cnt / pool_seeds
  int32_t chains, seeds;
};

struct ChainTablesOut {
  int32_t* chain_cnt;     // per read
  int32_t* chain_base;    // first chain of read r (the batch's chain limit is 2^31: the caller refuses a larger total)
  long long* reg_base;    // first output slot of read r == the seeds before it
  int32_t* seed_cnt;      // per chain
  long long* seed_base;   // first seed of chain c
  long long* seed_rbeg;   // per seed: bpsw_seed_t unzipped
  int32_t* seed_qbeg;
  int32_t* seed_len;
};

// read r's rows of every table; returns the largest seed count of its chains (0: the read has none)
BPSW_TABLES_HD int chain_tables_read(const ChainWhere* where, const int32_t* pool_cnt, const bpsw_seed_t* pool_seeds, long long r,
                                     long long chain_at, long long seed_at, const ChainTablesOut& T) {
  const long long cnt_at = where[r].cnt_at, from = where[r].seed_at;
  const int chains = where[r].chains;
  T.chain_cnt[r] = chains;
  T.chain_base[r] = (int32_t)chain_at;
  T.reg_base[r] = seed_at;
  int largest = 0;
  long long s = 0;
  for (int k = 0; k < chains; ++k) {
    const int ns = pool_cnt[cnt_at + k];
    T.seed_cnt[chain_at + k] = ns;
    T.seed_base[chain_at + k] = seed_at + s;
    for (int i = 0; i < ns; ++i, ++s) {
      const bpsw_seed_t* p = pool_seeds + from + s;
      T.seed_rbeg[seed_at + s] = p->rbeg;
      T.seed_qbeg[seed_at + s] = p->qbeg;
      T.seed_len[seed_at + s] = p->len;
    }
    largest = ns > largest ? ns : largest;
  }
  return largest;
}

}  // namespace bpsw
