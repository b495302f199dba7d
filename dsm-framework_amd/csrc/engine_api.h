// engine_api.h -- what the C entry points (abi.hip) and the server side (server.hip) see of the frontier engine (engine.hip).
#pragma once
#include <string>
#include <vector>

#include "common.h"

// A sample given as an already enumerated trie: the byte stream an (unmodified reference) client sent to the server, parsed with
// TrieReader's token rules (TrieReader.h:32-106) into level arrays on the device, in the order the nodes appear = path order inside a level.
struct dsm_trie {
    int device = 0;
    dsm::u64 nodes = 0, maxfreq = 0;
    std::vector<dsm::u64> level_off;  // level l holds nodes [level_off[l], level_off[l+1]); level 0 = the root
    dsm::u64* d_freq = nullptr;       // per node
    dsm::u8* d_pl = nullptr;          // bits 0-3 children present, bits 4-6 left-char code
    dsm::u32* d_fc = nullptr;         // index of the first child inside the next level
};

namespace dsm {

// a miner behind dsm_miner*: positions are 32 or 64 bits wide inside (MinerT<P>, engine.hip)
struct MinerBase {
    virtual ~MinerBase() {}
    virtual bool stream_mode() const = 0;
    virtual int run(const char* prefix, dsm_tuple_sink ts, dsm_byte_sink bs, void* ctx, dsm_stats* out) = 0;
    virtual int run_many(const char* const* prefixes, int n, dsm_tuple_sink ts, dsm_byte_sink bs, void* ctx, dsm_stats* out,
                         dsm_prefix_byte_sink ps = nullptr, dsm_text_sink xs = nullptr) = 0;
};
bool need_wide(dsm_index* const* idx, int n, const dsm_params* p);
MinerBase* miner_create(dsm_index* const* idx, int n, const dsm_params& p, bool stream_mode, int* rc);
int mine_once(dsm_index* const* idx, int n, const dsm_params* p, dsm_tuple_sink sink, void* ctx, dsm_stats* stats);
int enumerate_once(const dsm_index* idx, const char* prefix, u32 fmin, u32 maxdepth, dsm_byte_sink sink, void* ctx, dsm_stats* stats);
int merge_once(bool wide, dsm_trie* const* tr, int n, const dsm_params* p, dsm_tuple_sink sink, void* ctx, dsm_stats* stats);

// ---- how one engine run (Engine<P>::run) cuts a prefix's trie ----
// Used when a prefix is split because a level did not fit (MinerT::run_auto) and by the server side's passes.  Reader-set iteration
// orders depend on the whole sibling structure above a node, so a sub-prefix run must start from the order its root had in the
// unsplit trie (seed), captured by the shallow pass of the parent (capture).
struct NodeOrder {
    u32 depth = 0;
    std::vector<u32> sym;               // capture: symbol of each node at `depth`
    std::vector<std::vector<u16>> ord;  // capture: their orders; seed: ord[0]
};
struct RunOpts {
    bool emit = true;                  // this rank emits the prefix (tuples, or the wire stream)
    u32 emit_lo = 1, emit_hi = ~0u;    // only nodes with emit_lo <= depth <= emit_hi are filtered and emitted
    u32 expand_cap = ~0u;              // nodes at this depth or deeper are not expanded
    const NodeOrder* seed = nullptr;   // the order of the node at seed->depth
    NodeOrder* capture = nullptr;      // receives the symbols and orders of the nodes at capture->depth
    bool count = true;                 // `reported` counts the nodes of the depths emit_lo..emit_hi (not in a shallow pass)
    bool last = false;                 // the last run of a call: no next prefix hides its tuples' copies, they start as early as they can
};

// ---- the server side's engine runs (dsm_server, server.hip) ----
struct ServerEngines;  // the engines a server keeps between its runs (engine.hip)
ServerEngines* server_engines_create();
void server_engines_destroy(ServerEngines* e);
// One engine run over the given tries (sample id = position): capture (shallow pass, o.capture), a unit (o.emit_hi open: a unit that does
// not fit the buffers splits like any prefix) or the closing pass over the depths o.emit_lo..o.emit_hi.  which: 0 = an engine for this
// run only, 1 = the kept engine for the passes over the tops of the streams, 2 = the kept engine for units.
int server_run(bool wide, dsm_trie* const* tr, int n, const dsm_params& q, const std::string& prefix, dsm_tuple_sink sink, void* ctx,
               const RunOpts& o, dsm_stats* out, ServerEngines* keep = nullptr, int which = 0);

}  // namespace dsm
