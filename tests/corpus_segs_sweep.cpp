// Stand-alone sweep over the segment-table check of qpn_cut_chunks (qpnet_amd/csrc/corpus_segs.h): every valid table of a grid of geometries and row layouts
// must be accepted, and the same table with ONE field corrupted must be refused with the right code and a message that names the place.  Built with the
// host sanitizers and run as a child process by tests/test_corpus_segs_cpu.py; prints the number of tables checked.
#include "../qpnet_amd/csrc/corpus_segs.h"
#include <cstdlib>
#include <cstring>
#include <vector>

static long n_tables = 0;
static unsigned long long rng_state = 0x9E3779B97F4A7C15ULL;
static unsigned rnd(unsigned n) {      // xorshift: the sweep is the same on every machine
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)((rng_state >> 20) % n);
}

struct Table { CorpusSegsIn in; std::vector<qpn_corpus_seg> segs; std::vector<int32_t> row_first; };

static void expect(const Table& t, int want, const char* needle, const char* what) {
    char msg[256]; msg[0] = 0;
    ++n_tables;
    const int rc = corpus_segs_check(t.in, t.segs.data(), t.row_first.data(), msg, sizeof(msg));
    if (rc != want || (needle && !strstr(msg, needle))) {
        fprintf(stderr, "FAILED %s: rc = %d (want %d), message \"%s\" (want \"%s\") -- B=%d frames=%d U=%d n_aux=%d bl=%d n_segs=%lld\n", what, rc, want, msg,
                needle ? needle : "", t.in.B, t.in.frames, t.in.U, t.in.n_aux, t.in.bl, (long long)t.in.n_segs);
        exit(1);
    }
}

// a valid table the way the planner lays rows out: utterances of whole frames back to back in the arenas, a row starts at a random frame and runs on
// through the utterances behind it; its last segment carries the one extra sample (alone where the row's frames end with an utterance)
static Table make(int B, int frames, int U, int n_aux, int max_utt_frames) {
    Table t;
    std::vector<int> utt;      // frames per utterance
    int64_t total = 0;
    while (total < (int64_t)(frames + 2) * (B + 1) || utt.size() < 3) { const int f = 1 + (int)rnd((unsigned)max_utt_frames); utt.push_back(f); total += f; }
    t.in.n_frames = total; t.in.n_samples = total * U; t.in.B = B; t.in.frames = frames; t.in.U = U; t.in.n_aux = n_aux;
    t.in.bl = 1 + (int)rnd((unsigned)(frames * U));
    t.row_first.push_back(0);
    for (int b = 0; b < B; ++b) {
        int64_t at = rnd((unsigned)(total - frames - 1));      // first frame of the row: at least frames + 1 frames follow
        int need_f = frames; int64_t need_s = (int64_t)frames * U + 1;
        size_t u = 0; int64_t u0 = 0;
        while (u0 + utt[u] <= at) u0 += utt[u++];
        while (need_s > 0) {
            const int64_t left = u0 + utt[u] - at;              // frames left in this utterance
            qpn_corpus_seg s;
            s.sample0 = at * U; s.frame0 = at; s.factor0 = at;
            const int64_t ts = need_s < left * U ? need_s : left * U;
            const int64_t tf = need_f < left ? need_f : left;
            s.n_samples = (int32_t)ts; s.n_frames = (int32_t)tf;
            t.segs.push_back(s);
            need_s -= ts; need_f -= (int)tf;
            u0 += utt[u++]; at = u0;
        }
        t.row_first.push_back((int32_t)t.segs.size());
    }
    t.in.n_segs = (int64_t)t.segs.size();
    return t;
}

int main() {
    static const int geoms[][2] = {{5, 3}, {110, 39}, {1, 1}, {80, 28}};      // (U, n_aux)
    static const int frame_counts[] = {1, 2, 3, 7, 16, 17, 33, 190};
    static const int utt_frames[] = {1, 3, 40, 400};
    for (const auto& g : geoms) for (int frames : frame_counts) for (int maxf : utt_frames) for (int B = 1; B <= 4; ++B) for (int rep = 0; rep < 6; ++rep) {
        const Table ok = make(B, frames, g[0], g[1], maxf);
        expect(ok, QPN_OK, nullptr, "a valid table");
        const int row = (int)rnd((unsigned)B);
        const int k0 = ok.row_first[row], nk = ok.row_first[row + 1] - k0, j = (int)rnd((unsigned)nk), k = k0 + j;
        char place[48]; snprintf(place, sizeof(place), "row %d segment %d", row, j);
        char rowname[24]; snprintf(rowname, sizeof(rowname), "row %d:", row);
        Table t;
        // the scalars
        t = ok; t.in.U = 0; expect(t, QPN_EINVAL, "U must", "U = 0");
        t = ok; t.in.U = -3; expect(t, QPN_EINVAL, "U must", "U < 0");
        t = ok; t.in.n_aux = 0; expect(t, QPN_EINVAL, "n_aux", "n_aux = 0");
        t = ok; t.in.bl = 0; expect(t, QPN_EINVAL, "bl must", "bl = 0");
        t = ok; t.in.bl = frames * g[0] + 1; expect(t, QPN_EINVAL, "bl must", "bl = T + 1");
        t = ok; t.in.B = 0; expect(t, QPN_EINVAL, "B must", "B = 0");
        t = ok; t.in.frames = 0; expect(t, QPN_EINVAL, "frames must", "frames = 0");
        // a segment past either end of an arena
        t = ok; t.segs[k].sample0 = ok.in.n_samples - ok.segs[k].n_samples + 1; expect(t, QPN_ERANGE, place, "samples one past the arena end");
        t = ok; t.segs[k].sample0 = -1; expect(t, QPN_ERANGE, place, "sample0 < 0");
        t = ok; t.segs[k].sample0 = INT64_MAX; expect(t, QPN_ERANGE, place, "sample0 huge");
        t = ok; t.segs[k].frame0 = ok.in.n_frames - ok.segs[k].n_frames + 1; expect(t, QPN_ERANGE, place, "feature rows one past the arena end");
        t = ok; t.segs[k].frame0 = -1; expect(t, QPN_ERANGE, place, "frame0 < 0");
        t = ok; t.segs[k].frame0 = INT64_MAX; expect(t, QPN_ERANGE, place, "frame0 huge");
        t = ok; t.segs[k].factor0 = ok.in.n_frames - (ok.segs[k].n_samples + g[0] - 1) / g[0] + 1; expect(t, QPN_ERANGE, place, "factors one past the arena end");
        t = ok; t.segs[k].factor0 = -1; expect(t, QPN_ERANGE, place, "factor0 < 0");
        // counts
        t = ok; t.segs[k].n_samples = -1; expect(t, QPN_EINVAL, place, "n_samples < 0");
        t = ok; t.segs[k].n_frames = -1; expect(t, QPN_EINVAL, place, "n_frames < 0");
        t = ok; t.segs[k].n_samples = INT32_MAX; t.segs[k].sample0 = 0; expect(t, t.in.n_samples >= INT32_MAX ? QPN_EINVAL : QPN_ERANGE, nullptr, "n_samples huge");
        if (ok.segs[k].n_samples > 0) { t = ok; t.segs[k].n_samples -= 1; expect(t, QPN_EINVAL, rowname, "a row one sample short"); }
        t = ok; t.segs[k].sample0 = 0; t.segs[k].factor0 = 0; t.segs[k].n_samples += 1; expect(t, QPN_EINVAL, rowname, "a row one sample long");
        if (ok.segs[k].n_frames > 0) { t = ok; t.segs[k].n_frames -= 1; expect(t, QPN_EINVAL, rowname, "a row one feature row short"); }
        t = ok; t.segs[k].frame0 = 0; t.segs[k].n_frames += 1; expect(t, QPN_EINVAL, rowname, "a row one feature row long");
        // the row index
        t = ok; t.row_first[0] = 1; expect(t, QPN_EINVAL, "row_first", "row_first[0] != 0");
        t = ok; t.row_first[B] += 1; expect(t, QPN_EINVAL, "row_first", "row_first[B] != n_segs");
        t = ok; t.in.n_segs += 1; expect(t, QPN_EINVAL, "row_first", "n_segs off by one");
        if (B > 1) {
            const int r = 1 + (int)rnd((unsigned)(B - 1));
            t = ok; t.row_first[r] = ok.row_first[r + 1] + 1; expect(t, QPN_EINVAL, "monotone", "row_first not monotone");
            t = ok; t.row_first[r] = -1; expect(t, QPN_EINVAL, "monotone", "row_first negative");
            t = ok; t.row_first[r] = ok.row_first[r - 1]; expect(t, QPN_EINVAL, "row ", "an empty row");
        }
    }
    // NULL tables and a message buffer of no size
    { Table t = make(2, 3, 5, 3, 3); char c;
      if (corpus_segs_check(t.in, nullptr, t.row_first.data(), &c, 0) != QPN_EINVAL || corpus_segs_check(t.in, t.segs.data(), nullptr, nullptr, 16) != QPN_EINVAL) { fprintf(stderr, "FAILED NULL table\n"); return 1; }
      t.in.U = 0; if (corpus_segs_check(t.in, t.segs.data(), t.row_first.data(), nullptr, 0) != QPN_EINVAL) { fprintf(stderr, "FAILED no message buffer\n"); return 1; } }
    printf("CORPUS_SEGS_SWEEP_OK %ld\n", n_tables);
    return 0;
}
