// Host-only check of intrinsicavatar_amd/csrc/ia_scratch.h (built with -fsanitize=address,undefined by tests/test_scratch_cpu.py).
// Sequences of 1..12 pieces, sizes from {0, 1, 4, 255, 256, 257, 4096 + 12}, alignments from {4, 8, 16, 64, 256}, every misalignment
// 0..255 of the base: all sequences of one and two pieces, and pseudo-random longer ones.  For each: a measuring pass returns nullptr
// from every take; a carve hands out aligned, ordered, disjoint pieces inside [base, base + used()); used() of the carve is at most the
// measured need(base_align) for every base_align that divides the misalignment; fits() is false exactly from used() - 1 bytes down;
// every piece is written (the sanitizer sees a piece that leaves the allocation).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../intrinsicavatar_amd/csrc/ia_scratch.h"

static const size_t SIZES[] = {0, 1, 4, 255, 256, 257, 4096 + 12};
static const size_t ALIGNS[] = {4, 8, 16, 64, 256};
static const int NS = 7, NA = 5;

struct Piece { size_t size, align; };

static long long n_checked = 0;

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) {                                                                                \
            std::fprintf(stderr, "scratch_harness: line %d: %s failed (%zu pieces, misalignment %d)\n", __LINE__, #cond, seq.size(), mis); \
            std::exit(1);                                                                             \
        }                                                                                             \
    } while (0)

static size_t run(ia::Carver& c, const std::vector<Piece>& seq, std::vector<char*>* out)
{
    for (const Piece& p : seq) {
        char* q = c.take<char>(p.size, p.align);
        if (out) out->push_back(q);
    }
    return c.used();
}

static void check_sequence(const std::vector<Piece>& seq)
{
    int mis = -1;
    // measuring pass
    ia::Carver m(nullptr);
    std::vector<char*> none;
    const size_t measured = run(m, seq, &none);
    for (char* q : none) CHECK(q == nullptr);
    CHECK(m.fits());
    size_t max_align = 1, payload = 0;
    for (const Piece& p : seq) { if (p.align > max_align) max_align = p.align; payload += p.size; }
    CHECK(measured >= payload);
    CHECK(m.need(max_align) == measured && m.need(256) == measured && m.need(1) == measured + max_align - 1);

    const size_t worst = m.need(1);                                   // any base
    std::vector<char> buf(256 + 255 + worst + 1);
    char* aligned = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(buf.data()) + 255) & ~static_cast<uintptr_t>(255));
    for (mis = 0; mis < 256; mis++) {
        char* base = aligned + mis;
        ia::Carver c(base, worst);
        std::vector<char*> ptr;
        const size_t used = run(c, seq, &ptr);
        CHECK(c.used() == used && c.fits());
        CHECK(used <= worst);
        for (size_t ba : {size_t(1), size_t(4), size_t(8), size_t(16), size_t(64), size_t(256)})
            if (mis % ba == 0) CHECK(used <= m.need(ba));
        if (mis == 0) CHECK(used == measured);
        char* end = base;
        for (size_t i = 0; i < seq.size(); i++) {
            CHECK(ptr[i] != nullptr);
            CHECK(reinterpret_cast<uintptr_t>(ptr[i]) % seq[i].align == 0);
            CHECK(ptr[i] >= end);                                     // ordered and disjoint
            CHECK(static_cast<size_t>(ptr[i] - end) < seq[i].align);  // no more padding than the alignment asks for
            end = ptr[i] + seq[i].size;
            std::memset(ptr[i], 0xA5, seq[i].size);
        }
        CHECK(end == base + used);
        // fits(): true with exactly used() bytes, false with one fewer
        ia::Carver exact(base, used);
        run(exact, seq, nullptr);
        CHECK(exact.fits());
        if (used > 0) {
            ia::Carver tight(base, used - 1);
            run(tight, seq, nullptr);
            CHECK(!tight.fits());
        }
        n_checked++;
    }
}

int main()
{
    std::vector<Piece> seq;
    // every sequence of one and of two pieces
    for (int a = 0; a < NS * NA; a++) {
        seq = {{SIZES[a % NS], ALIGNS[a / NS]}};
        check_sequence(seq);
        for (int b = 0; b < NS * NA; b++) {
            seq = {{SIZES[a % NS], ALIGNS[a / NS]}, {SIZES[b % NS], ALIGNS[b / NS]}};
            check_sequence(seq);
        }
    }
    // longer ones: a fixed pseudo-random choice, every length 3 .. 12
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto next = [&state](int n) { state = state * 6364136223846793005ull + 1442695040888963407ull; return (int)((state >> 33) % (uint64_t)n); };
    for (int len = 3; len <= 12; len++)
        for (int rep = 0; rep < 60; rep++) {
            seq.clear();
            for (int i = 0; i < len; i++) seq.push_back({SIZES[next(NS)], ALIGNS[next(NA)]});
            check_sequence(seq);
        }
    // typed pieces: count is in elements
    {
        int mis = 0;
        alignas(256) static unsigned char area[1024];
        ia::Carver c(area, sizeof(area));
        uint64_t* a = c.take<uint64_t>(3, 8);
        uint16_t* b = c.take<uint16_t>(5, 4);
        float* d = c.take<float>(7);
        CHECK(reinterpret_cast<unsigned char*>(a) == area && reinterpret_cast<unsigned char*>(b) == area + 24);
        CHECK(reinterpret_cast<unsigned char*>(d) == area + 256 && c.used() == 256 + 28 && c.fits());
    }
    std::printf("scratch_harness OK: %lld carves\n", n_checked);
    return 0;
}
