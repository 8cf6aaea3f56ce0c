// CPU: the host arithmetic of the member decode's stages (libflate_amd/csrc/lfx_stages.h) over seeded random ranges —
// the pieces of a range tile it exactly (no gap, no overlap, interior cuts a multiple of 64 bits behind the range's start,
// warm-ups that never reach in front of it), their number is the one the split formula gives, and the storing scan's lane
// regions never overlap; the range a member's walk may end in equals a plain re-statement over random candidate lists; and
// the parts of emit_round's d_dec_tmp never overlap, for every job count up to 5000.
#include <cstdio>
#include <random>

#include "../../libflate_amd/csrc/lfx_stages.h"

using namespace lfx;

// the pieces jobs[from, ..) of [s0, s1): returns how many, or -1 with a message
static int check_tiling(const std::vector<BlkJob> &jobs, size_t from, uint64_t s0, uint64_t s1, uint64_t overlap, int it) {
    uint64_t at = s0;
    for (size_t q = from; q < jobs.size(); q++) {
        const BlkJob &j = jobs[q];
        const uint64_t lo = q == from ? s0 : j.lo_bit;
        if (j.start_bit != s0 || j.piece != 1) { printf("case %d piece %zu: not a piece of its block\n", it, q - from); return -1; }
        if (lo != at) { printf("case %d piece %zu: starts at %llu, the one before ended at %llu\n", it, q - from, (unsigned long long)lo, (unsigned long long)at); return -1; }
        if (j.end_bit <= lo && !(q == from && s1 == s0)) { printf("case %d piece %zu: empty\n", it, q - from); return -1; }
        // (piece 0 starts behind the header like any job; the others at a cut, with a warm-up that stays inside the range)
        if (q == from ? (j.lo_bit != 0 || j.warm_bit != 0) : (j.warm_bit != lo - overlap || j.warm_bit < s0 || (lo - s0) % 64 != 0)) {
            printf("case %d piece %zu: cut or warm-up wrong\n", it, q - from);
            return -1;
        }
        at = j.end_bit;
    }
    if (at != s1) { printf("case %d: the pieces end at %llu, the range at %llu\n", it, (unsigned long long)at, (unsigned long long)s1); return -1; }
    return (int)(jobs.size() - from);
}

// member_walk_limit, re-stated: the first candidate behind `data`, the walk's byte budget from the member's start, the input's end
static uint64_t plain_walk_limit(const std::vector<uint64_t> &cand, size_t k, uint64_t data, uint64_t n) {
    uint64_t lim = n;
    if (cand[k] + MEMBER_WALK_BYTES < lim) lim = cand[k] + MEMBER_WALK_BYTES;
    for (uint64_t x : cand)
        if (x > data) { if (x < lim) lim = x; break; }
    return lim;
}

int main() {
    std::mt19937_64 rng(11), rng2(12);      // (rng2: the checks added later draw from a stream of their own)
    int cases = 0;
    int seen_eq = 0, seen_last = 0, seen_near_end = 0, seen_nothing = 0, seen_next = 0, seen_budget = 0;
    for (int it = 0; it < 20000; it++) {
        // a stream of `span` bits for `n_cu` CUs, a candidate range inside it
        const int n_cu = (int)(1 + rng() % 320);
        const uint64_t span = (64 + rng() % (1ull << (10 + rng() % 26)));
        const uint64_t nc = 1 + rng() % 100;
        const uint64_t want = rng() & 1 ? 2ull * (uint64_t)n_cu : (uint64_t)std::max<int64_t>(2ll * n_cu - (int64_t)nc, (int64_t)nc);
        const uint64_t piece = piece_bits(span, want), overlap = piece_overlap(piece);
        if (piece < (256ull << 10) || piece > (4ull << 20) || piece % 64) { printf("case %d: piece size %llu\n", it, (unsigned long long)piece); return 1; }
        const uint64_t first = rng() % 4096;
        const uint64_t s0 = first + rng() % span, len = 1 + rng() % (first + span - s0), s1 = s0 + len;
        // ---- the even split of a candidate range
        std::vector<BlkJob> jobs(rng() % 3);        // (appended behind what is there)
        const size_t from = jobs.size();
        add_pieces(jobs, s0, s1, piece, overlap);
        const int np = check_tiling(jobs, from, s0, s1, overlap, it);
        if (np < 0) return 1;
        // the count: enough pieces of at most `piece` bits, the range split evenly among them and rounded up to 64 bits
        const uint64_t np0 = std::max<uint64_t>((len + piece - 1) / piece, 1);
        const uint64_t pb = std::max<uint64_t>(((len + np0 - 1) / np0 + 63) & ~63ull, 64);
        const uint64_t expect = std::max<uint64_t>((len + pb - 1) / pb, 1);
        if ((uint64_t)np != expect) { printf("case %d: %d pieces, the formula gives %llu\n", it, np, (unsigned long long)expect); return 1; }
        for (size_t q = from; q < jobs.size(); q++)
            if (jobs[q].end_bit - (q == from ? s0 : jobs[q].lo_bit) > pb) { printf("case %d: a piece longer than the even share\n", it); return 1; }
        // ---- the fixed split of the stream's rest (the block-by-block walk)
        std::vector<BlkJob> fixed;
        add_fixed_pieces(fixed, s0, s1, piece, overlap);
        const int nf = check_tiling(fixed, 0, s0, s1, overlap, it);
        if (nf < 0) return 1;
        if ((uint64_t)nf != (len + piece - 1) / piece) { printf("case %d: %d fixed pieces\n", it, nf); return 1; }
        // ---- lane regions of a scan's jobs: candidate ranges, some of them overlapping alternatives
        std::vector<uint64_t> starts;
        uint64_t b = first;
        const uint64_t end_bits = first + span;
        while (b < end_bits && starts.size() < 300) { starts.push_back(b); b += 1 + rng() % (span / (1 + rng() % 64) + 1); }
        std::vector<BlkJob> bj(starts.size());
        for (size_t i = 0; i < starts.size(); i++) bj[i] = BlkJob{starts[i], i + 1 < starts.size() ? starts[i + 1] : end_bits};
        const std::vector<int32_t> alt = add_alt_jobs(bj, starts, end_bits, span / 8);
        for (size_t i = 0; i < alt.size(); i++)
            if (alt[i] >= 0 && ((size_t)alt[i] < starts.size() || (size_t)alt[i] >= bj.size() || bj[alt[i]].start_bit != starts[i] ||
                                bj[alt[i]].end_bit <= bj[i].end_bit)) { printf("case %d: alternative job of candidate %zu\n", it, i); return 1; }
        if (bj.size() - starts.size() > starts.size() / 4 + 5) { printf("case %d: too many alternative jobs\n", it); return 1; }
        const bool tight = rng() & 1;
        const uint64_t dwords = plan_store_regions(bj.data(), (uint32_t)bj.size(), tight);
        uint64_t at = 0;
        for (const BlkJob &j : bj) {           // (laid out in job order: disjoint iff each starts where the one before ended)
            const uint64_t slice = (j.end_bit - j.start_bit + 1023) / 1024;
            if (j.temp_off != at || j.cap % 4 || j.cap < slice / (tight ? 16 : 2) + 448) { printf("case %d: region of a job\n", it); return 1; }
            at = j.temp_off + 1024ull * j.cap;
        }
        if (at != dwords) { printf("case %d: regions take %llu dwords, reported %llu\n", it, (unsigned long long)at, (unsigned long long)dwords); return 1; }
        clear_store_regions(bj.data(), (uint32_t)bj.size());
        for (const BlkJob &j : bj) if (j.temp_off || j.cap) { printf("case %d: region not cleared\n", it); return 1; }
        // ---- the range a member's walk may end in: sorted candidates (gaps from a few bytes to several walk budgets), a
        // header of 0 bytes up to more than the budget, an input that ends anywhere from inside the header on
        {
            std::vector<uint64_t> cand;
            uint64_t at = rng2() % 4096;
            const size_t ncand = 1 + rng2() % 40;
            for (size_t i = 0; i < ncand; i++) { cand.push_back(at); at += 1 + rng2() % (1ull << (2 + rng2() % 23)); }
            const size_t k = rng2() % 4 == 0 ? ncand - 1 : rng2() % ncand;
            uint64_t hdr = rng2() % 4 == 0 ? 0 : 10 + rng2() % (1ull << (4 + rng2() % 20));
            if (k + 1 < ncand && rng2() % 8 == 0) hdr = cand[k + 1] - cand[k];         // (the data starts AT a later candidate)
            const uint64_t data = cand[k] + hdr;
            const uint64_t n = rng2() % 4 == 0 ? cand[k] + 1 + rng2() % (hdr + 4096) : cand.back() + 1 + rng2() % (16ull << 20);
            const uint64_t lim = member_walk_limit(cand, k, data, n), want_lim = plain_walk_limit(cand, k, data, n);
            if (lim != want_lim) { printf("case %d: walk limit %llu, re-stated %llu\n", it, (unsigned long long)lim, (unsigned long long)want_lim); return 1; }
            if (lim > n || lim > cand[k] + MEMBER_WALK_BYTES) { printf("case %d: walk limit out of range\n", it); return 1; }
            seen_eq += std::binary_search(cand.begin(), cand.end(), data);
            seen_last += k + 1 == ncand;
            seen_near_end += n < cand[k] + MEMBER_WALK_BYTES && lim == n;
            seen_nothing += lim <= data;
            seen_next += lim < n && lim < cand[k] + MEMBER_WALK_BYTES;
            seen_budget += lim == cand[k] + MEMBER_WALK_BYTES && lim < n;
        }
        cases++;
    }
    if (!seen_eq || !seen_last || !seen_near_end || !seen_nothing || !seen_next || !seen_budget) {
        printf("walk limit: a kind of case never came up (%d %d %d %d %d %d)\n", seen_eq, seen_last, seen_near_end, seen_nothing, seen_next, seen_budget);
        return 1;
    }
    // ---- emit_round's d_dec_tmp: 64 flag bytes, the job flags, the jobs — disjoint, the jobs 8-byte aligned, and no larger
    // than sizeof(BlkEmit) * ne + 4 * ne + 128 (what the callers of the round reserved before the layout had a home)
    int layouts = 0;
    for (uint32_t ne = 1; ne <= 5000; ne++) {
        const EmitTmp t = emit_tmp_layout(ne);
        const bool disjoint = t.flags + 64 <= t.job_flags && t.job_flags + 4ull * ne <= t.jobs && t.jobs + sizeof(BlkEmit) * (uint64_t)ne <= t.total;
        if (!disjoint || t.flags % 4 || t.job_flags % 4 || t.jobs % 8 || t.total > sizeof(BlkEmit) * (uint64_t)ne + 4ull * ne + 128) {
            printf("layout of %u emit jobs: flags %llu, job flags %llu, jobs %llu, total %llu\n", ne, (unsigned long long)t.flags,
                   (unsigned long long)t.job_flags, (unsigned long long)t.jobs, (unsigned long long)t.total);
            return 1;
        }
        layouts++;
    }
    printf("plan_stages ok: %d cases, %d layouts\n", cases, layouts);
    return 0;
}
