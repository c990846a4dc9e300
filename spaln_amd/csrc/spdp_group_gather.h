// spdp_group_gather.h -- the results of a group's members put back into the caller's order (spdp_group.cpp).
//
// A group call shards its n queries over the members; member r gets the queries idx[r] (caller numbers, ascending) and
// answers for them numbered 0 .. idx[r].size() - 1.  What comes back has one of three shapes:
//   1. a value per query (a score, a status, a record of out_cap ints, a tail record): scatter / pick;
//   2. a list per query, the lists pooled one behind the other (hits, genes, loci): Part::off + Part::rec -> gather_lists;
//   3. a pooled side array that the list's records address with an offset field (the corners of a hit, the exons of a gene,
//      the HSPs of a locus): Part::side, rebased by gather_lists while it copies.
// The caller's pools are the members' lists concatenated in the CALLER's query order with the offsets counted again, which is
// what the single-context entry writes for the same queries in one call.
// Plain C++: no HIP, no context types; the record type and its fields (offset, count, query number) are template arguments.
// tests/group_gather_host_check.cpp drives it under the sanitizers.
#ifndef SPDP_GROUP_GATHER_H_
#define SPDP_GROUP_GATHER_H_
#include <cstddef>
#include <cstdint>
#include <vector>

namespace spdp_gather {

// where query i of the caller went: member, and its number there (member < 0: nobody served it -- its list stays empty)
struct Place { int member = -1; int k = 0; };

inline std::vector<Place> places(int n, const std::vector<std::vector<int>>& idx)
{
    std::vector<Place> at((size_t) (n > 0 ? n : 0));
    for (size_t r = 0; r < idx.size(); ++r)
        for (size_t k = 0; k < idx[r].size(); ++k)
            if (idx[r][k] >= 0 && idx[r][k] < n) { at[(size_t) idx[r][k]].member = (int) r; at[(size_t) idx[r][k]].k = (int) k; }
    return at;
}

// ---- shape 1: `stride` values per query ------------------------------------------------------------------------------------
// a member's inputs picked out of the caller's array (all may be null: nothing is picked, the vector stays empty)
template <typename T>
std::vector<T> pick(const std::vector<int>& idx, const T* all, size_t stride = 1)
{
    std::vector<T> mine;
    if (!all) return mine;
    mine.reserve(idx.size() * stride);
    for (int i : idx) mine.insert(mine.end(), all + (size_t) i * stride, all + ((size_t) i + 1) * stride);
    return mine;
}
// a member's results written to the caller's slots (out may be null: a result the caller did not ask for)
template <typename T>
void scatter(const std::vector<int>& idx, const T* mine, T* out, size_t stride = 1)
{
    if (!out || !mine) return;
    for (size_t k = 0; k < idx.size(); ++k)
        for (size_t j = 0; j < stride; ++j) out[(size_t) idx[k] * stride + j] = mine[k * stride + j];
}

// ---- shapes 2 and 3 ------------------------------------------------------------------------------------------------------------
// what one member returned for its shard: the lists of its queries (query k: rec[off[k] .. off[k + 1])) and the side array its
// records point into.  S = char and an empty side for a list without one.
template <typename R, typename S = char>
struct Part {
    std::vector<int64_t> off;           // cnt + 1 entries; empty: the member served nothing
    std::vector<R> rec;
    std::vector<S> side;
};

// the offsets of a member's lists where the entry marks every record with its query instead (spdp_blk_find: the records lie
// query by query, ascending).  A record whose number is outside 0 .. cnt - 1 is counted for nobody.
template <typename R, typename Q>
std::vector<int64_t> offsets_by_query(const R* rec, int64_t n_rec, int cnt, Q R::*query)
{
    std::vector<int64_t> off((size_t) (cnt > 0 ? cnt : 0) + 1, 0);
    for (int64_t j = 0; j < n_rec; ++j) {
        const int64_t q = (int64_t) (rec[j].*query);
        if (q >= 0 && q < cnt) ++off[(size_t) q + 1];
    }
    for (size_t k = 1; k < off.size(); ++k) off[k] += off[k - 1];
    return off;
}

// how much of a member's side array its records use (an entry hands out a malloc'ed pool without its length)
template <typename R, typename O, typename N>
size_t side_extent(const R* rec, int64_t n_rec, O R::*side_off, N&& side_count)
{
    size_t e = 0;
    for (int64_t j = 0; j < n_rec; ++j) {
        const int64_t c = (int64_t) side_count(rec[j]);
        if (c > 0 && (size_t) (rec[j].*side_off + c) > e) e = (size_t) (rec[j].*side_off + c);
    }
    return e;
}

struct Totals { size_t rec = 0, side = 0; };

// what the caller's pools must hold: the records of every served query, the side entries those records count
template <typename R, typename S, typename N>
Totals totals(const std::vector<Place>& at, const std::vector<Part<R, S>>& part, N&& side_count)
{
    Totals t;
    for (const Place& p : at) {
        if (p.member < 0 || (size_t) p.member >= part.size()) continue;
        const Part<R, S>& P = part[(size_t) p.member];
        if ((size_t) p.k + 1 >= P.off.size()) continue;
        for (int64_t j = P.off[(size_t) p.k]; j < P.off[(size_t) p.k + 1]; ++j) {
            ++t.rec;
            const int64_t c = (int64_t) side_count(P.rec[(size_t) j]);
            if (c > 0) t.side += (size_t) c;
        }
    }
    return t;
}
template <typename R, typename S>
Totals totals(const std::vector<Place>& at, const std::vector<Part<R, S>>& part)
{
    return totals(at, part, [](const R&) { return 0; });
}

// the members' lists in the caller's query order: out_off[n + 1] (may be null: one record per query, or the records say whose
// they are), out_rec and out_side sized by totals().  Every record's side entries are copied behind those of the record before
// it and side_off is set to where they now begin -- for a record without side entries too, as the single-context entries count.
// renumber(record, caller's query number) is called on every copied record (the query field of a locus).
template <typename R, typename S, typename O, typename N, typename F>
void gather_lists(const std::vector<Place>& at, const std::vector<Part<R, S>>& part, int64_t* out_off, R* out_rec, S* out_side,
                  O R::*side_off, N&& side_count, F&& renumber)
{
    int64_t k = 0, o = 0;
    if (out_off) out_off[0] = 0;
    for (size_t i = 0; i < at.size(); ++i) {
        const Place& p = at[i];
        if (p.member >= 0 && (size_t) p.member < part.size() && (size_t) p.k + 1 < part[(size_t) p.member].off.size()) {
            const Part<R, S>& P = part[(size_t) p.member];
            for (int64_t j = P.off[(size_t) p.k]; j < P.off[(size_t) p.k + 1]; ++j, ++k) {
                R rec = P.rec[(size_t) j];
                const int64_t c = (int64_t) side_count(rec);
                for (int64_t x = 0; x < c; ++x) out_side[o + x] = P.side[(size_t) (rec.*side_off + x)];
                rec.*side_off = (O) o;
                if (c > 0) o += c;
                renumber(rec, (int) i);
                out_rec[k] = rec;
            }
        }
        if (out_off) out_off[i + 1] = k;
    }
}
// a list without a side array (a value per record that lies pooled beside the records: SpdpMapGene's `part`)
template <typename R>
void gather_lists(const std::vector<Place>& at, const std::vector<Part<R, char>>& part, int64_t* out_off, R* out_rec)
{
    int64_t k = 0;
    if (out_off) out_off[0] = 0;
    for (size_t i = 0; i < at.size(); ++i) {
        const Place& p = at[i];
        if (p.member >= 0 && (size_t) p.member < part.size() && (size_t) p.k + 1 < part[(size_t) p.member].off.size()) {
            const Part<R, char>& P = part[(size_t) p.member];
            for (int64_t j = P.off[(size_t) p.k]; j < P.off[(size_t) p.k + 1]; ++j, ++k) out_rec[k] = P.rec[(size_t) j];
        }
        if (out_off) out_off[i + 1] = k;
    }
}

}   // namespace spdp_gather
#endif /* SPDP_GROUP_GATHER_H_ */
