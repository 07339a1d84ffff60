// step_key_check.cpp -- host check of the graph keys (nano_amd/csrc/step_spec.h), run by tests/test_step_key.py:
//   g++ -std=c++17 -O1 -o step_key_check tools/step_key_check.cpp && ./step_key_check <max_seq_len>
// Enumerates a table of steps -- the three kinds of rows as the fast path runs them and SEQS as the reference-order step does, nb, modes,
// causal, hints, slots, LoRA / stamps / skip_embed on and off, the four key_kinds -- and checks that
//   * two steps of one family get the same key exactly when they agree in every field that family's nodes depend on (the signatures
//     below are written out by hand, family by family: they are the specification, step_key the implementation),
//   * keys of different families never collide, and a ragged pass has no key,
//   * a field value one past its width is "no key", and so is the fast step's SEQS in a slot other than 0.
#include <stdio.h>
#include <stdlib.h>

#include <array>
#include <map>
#include <type_traits>
#include <vector>

#include "../nano_amd/csrc/step_spec.h"

static_assert(std::is_trivially_copyable<StepSpec>::value, "a StepSpec is a value: graph lambdas capture it by copy");

struct Case { StepSpec s; bool ordered; uint32_t key_kind; bool lora, stamps; };
using Sig = std::array<uint64_t, 8>;                      // [0] = the family, then what the family distinguishes

// what each family's key distinguishes: what its captured nodes depend on beyond the model's creation-time facts and drop_graphs()
static Sig signature(const Case &c) {
    const StepSpec &s = c.s;
    if (c.ordered) return { FAMILY_ORDERED, s.slot, s.nb, s.is_causal, s.mode, 0, 0, 0 };
    if (s.rows == StepSpec::CHUNK) return { FAMILY_CHUNK, c.key_kind, c.lora, s.slot, s.range_hint, s.nb, 0, 0 };
    return { FAMILY_FAST, c.stamps, (uint64_t)(s.skip_embed && s.mode == MODE_LOOP), c.lora, s.range_hint, s.nb, s.is_causal, s.mode };
}
static uint64_t key_of(const Case &c) { return step_key(c.s, c.ordered, c.key_kind, c.lora, c.stamps); }

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

int main(int argc, char **argv) {
    const uint32_t S = argc > 1 ? (uint32_t)strtoul(argv[1], nullptr, 0) : 40960u;
    const uint32_t nbs[] = { 1, 8, 9, 64 }, hints[] = { 64, 80, 2048, S }, slots[] = { 0, 1, 63 };
    static const RowGroup group{ 0, 1, 64 };
    std::vector<Case> cases;
    for (uint32_t nb : nbs) for (uint32_t mode = 0; mode <= 5; mode++) for (uint32_t causal = 0; causal <= 1; causal++) for (uint32_t hint : hints)
        for (uint32_t flags = 0; flags < 8; flags++) {
            const bool lora = flags & 1, stamps = flags & 2, skip = flags & 4;
            {   // the fast decode step: slot 0
                Case c{ StepSpec::seqs(nb, causal, mode, hint), false, 0, lora, stamps };
                c.s.skip_embed = skip;
                cases.push_back(c);
            }
            for (uint32_t slot : slots) {
                {   // the reference-order step in slot0 = slot
                    Case c{ StepSpec::seqs(nb, causal, mode, hint, slot), true, 0, lora, stamps };
                    c.s.skip_embed = skip;
                    cases.push_back(c);
                }
                for (uint32_t kind = 0; kind < 4; kind++) {   // a chunk of the call kinds (mode and causal vary in the spec: its key does not read them)
                    Case c{ StepSpec::chunk(slot, nb, mode, hint, kind == 1), false, kind, lora, stamps };
                    c.s.is_causal = causal; c.s.skip_embed = skip;
                    cases.push_back(c);
                }
            }
        }
    // same key <=> same signature: both maps must be functions
    std::map<uint64_t, Sig> by_key;
    std::map<Sig, uint64_t> by_sig;
    size_t families[4] = { 0, 0, 0, 0 };
    for (const Case &c : cases) {
        const uint64_t key = key_of(c);
        const Sig sig = signature(c);
        CHECK(key != STEP_NO_KEY, "no key for a step of family %llu (nb %u mode %u hint %u slot %u)", (unsigned long long)sig[0], c.s.nb, c.s.mode, c.s.range_hint, c.s.slot);
        auto k = by_key.emplace(key, sig);
        CHECK(k.first->second == sig, "key %016llx is shared by two steps that differ (families %llu and %llu)", (unsigned long long)key, (unsigned long long)k.first->second[0], (unsigned long long)sig[0]);
        auto g = by_sig.emplace(sig, key);
        CHECK(g.first->second == key, "two steps that agree in every field of family %llu got keys %016llx and %016llx", (unsigned long long)sig[0], (unsigned long long)g.first->second, (unsigned long long)key);
        CHECK(((key >> KEY_FAMILY.shift) & 3u) == sig[0], "key %016llx does not carry family %llu", (unsigned long long)key, (unsigned long long)sig[0]);
        families[sig[0]]++;
    }
    CHECK(by_key.size() == by_sig.size(), "%zu keys for %zu signatures", by_key.size(), by_sig.size());
    // a ragged pass has no key; neither has a chunk or ragged pass under the reference-order step, nor the fast step outside slot 0
    CHECK(step_key(StepSpec::ragged(3, MODE_VERIFY, nullptr, &group, 1, false), false, 3, false, false) == STEP_NO_KEY, "a ragged pass got a key");
    CHECK(step_key(StepSpec::chunk(0, 64, MODE_NOCLS, 64, false), true, 0, false, false) == STEP_NO_KEY, "a chunk got a reference-order key");
    CHECK(step_key(StepSpec::seqs(1, 1, MODE_LOGITS, 64, 1), false, 0, false, false) == STEP_NO_KEY, "the fast step got a key in slot 1");
    // one past each field's width: no key (and the largest value that fits: a key)
    struct Edge { const char *name; KeyField f; uint32_t family; };      // family: which kind of step carries the field (0: all three)
    const Edge edges[] = { { "nb", KEY_NB, 0 }, { "mode", KEY_MODE, FAMILY_FAST }, { "mode", KEY_MODE, FAMILY_ORDERED }, { "is_causal", KEY_CAUSAL, FAMILY_FAST },
                           { "is_causal", KEY_CAUSAL, FAMILY_ORDERED }, { "slot", KEY_SLOT, FAMILY_CHUNK }, { "slot", KEY_SLOT, FAMILY_ORDERED },
                           { "range_hint", KEY_HINT, FAMILY_FAST }, { "range_hint", KEY_HINT, FAMILY_CHUNK }, { "key_kind", KEY_KIND, FAMILY_CHUNK } };
    size_t n_edges = 0;
    for (const Edge &e : edges)
        for (uint32_t family = FAMILY_FAST; family <= FAMILY_ORDERED; family++) {
            if (e.family && e.family != family) continue;
            for (int over = 0; over <= 1; over++) {
                const uint32_t v = (uint32_t)((1ull << e.f.width) - 1 + over);
                Case c{ family == FAMILY_CHUNK ? StepSpec::chunk(2, 64, MODE_NOCLS, 128, false) : StepSpec::seqs(4, 1, MODE_ARGMAX, 128, family == FAMILY_ORDERED ? 2u : 0u),
                        family == FAMILY_ORDERED, family == FAMILY_CHUNK ? 1u : 0u, false, false };
                if (e.f.shift == KEY_NB.shift) c.s.nb = v;
                else if (e.f.shift == KEY_MODE.shift) c.s.mode = v;
                else if (e.f.shift == KEY_CAUSAL.shift) c.s.is_causal = v;
                else if (e.f.shift == KEY_SLOT.shift) c.s.slot = v;
                else if (e.f.shift == KEY_HINT.shift) c.s.range_hint = v;
                else c.key_kind = v;
                const uint64_t key = key_of(c);
                CHECK((key == STEP_NO_KEY) == (over == 1), "%s = %u in family %u: key %016llx", e.name, v, family, (unsigned long long)key);
                // ... and a value that fits stays inside its field: every other field reads as it does with the field at 0
                if (!over) {
                    Case z = c;
                    if (e.f.shift == KEY_NB.shift) z.s.nb = 0; else if (e.f.shift == KEY_MODE.shift) z.s.mode = 0; else if (e.f.shift == KEY_CAUSAL.shift) z.s.is_causal = 0;
                    else if (e.f.shift == KEY_SLOT.shift) z.s.slot = 0; else if (e.f.shift == KEY_HINT.shift) z.s.range_hint = 0; else z.key_kind = 0;
                    const uint64_t mask = ((1ull << e.f.width) - 1) << e.f.shift;
                    CHECK((key & ~mask) == (key_of(z) & ~mask) && ((key & mask) >> e.f.shift) == v, "%s = %u in family %u spills out of its field", e.name, v, family);
                }
                n_edges++;
            }
        }
    // the fields do not overlap and fit 64 bits
    const KeyField all[] = { KEY_NB, KEY_MODE, KEY_CAUSAL, KEY_LORA, KEY_SKIP_EMBED, KEY_STAMPS, KEY_SLOT, KEY_HINT, KEY_KIND, KEY_FAMILY };
    uint64_t used = 0;
    for (const KeyField &f : all) {
        const uint64_t mask = ((1ull << f.width) - 1) << f.shift;
        CHECK(f.shift + f.width <= 64 && !(used & mask), "field at bit %u overlaps another", f.shift);
        used |= mask;
    }
    printf("%zu steps (%zu fast, %zu chunk, %zu ordered), %zu distinct keys, %zu width edges, max_seq_len %u: %d failures\n", cases.size(), families[FAMILY_FAST],
           families[FAMILY_CHUNK], families[FAMILY_ORDERED], by_key.size(), n_edges, S, failures);
    return failures ? 1 : 0;
}
