"""The structure of a belief propagation set-up is pure host arithmetic over the compiled records
(numbskull_amd/csrc/nsk_bp_plan.h): which variables are clamped, every factor's distinct members and member records, the
table sizes, the directed edges, the per-variable edge lists with the binary variables first, the counts of nsk_bp_info and
every refusal.  The kernels trust these indices without a check.  A stand-alone program fills Compiled by hand and asserts
every array of the plan against values written out here: a factor that names a member twice, one with a clamped and a free
member, a function -1 factor, an isolated free variable and an id past the positions, with the evidence clamped and free
on the same records; free variables of cardinality 2, 3, NSK_ZLOCAL and NSK_ZLOCAL + 1; every refusal, with the texts
nsk_bp_setup gave when it built the structure itself, on a graph whose factor 0 is fine and whose factor 1 offends, beside
the nearest graph that is accepted.  Built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer
(-fno-sanitize-recover); a clean exit is the pass."""

import subprocess

import pytest

from test_alloc_ledger_cpu import CSRC, _compiler

PROGRAM = r"""
#undef NDEBUG
#include <array>
#include <cassert>
#include <cstdio>
#include "nsk_bp_plan.h"

using namespace nsk;
typedef std::vector<int32_t> I32;
typedef std::vector<long long> I64;
typedef std::vector<std::array<int32_t, 2>> Members;       // {internal id, dense_equal_to}

// variable v has internal id v; the ids below npos have a position and its isEvidence byte (the bits above it are not read)
struct Graph {
    Compiled c;
    Graph(const I32 &card, const I32 &evid, int64_t npos) {
        c.nvar = c.nid = (int64_t)card.size();
        c.npos = npos;
        c.nweight = 2;
        c.v_card_i = card;
        for (size_t v = 0; v < card.size(); v++) c.iid.push_back((int32_t)v);
        for (int64_t i = 0; i < npos; i++) c.p_info.push_back((uint32_t)evid[(size_t)i] | 0x300u);
    }
    // at: the record's first member position where it is not the next one
    void factor(int fn, int arity, int weight, const Members &m, int at = -1000) {
        const uint32_t rec[4] = {(uint32_t)arity << 8 | (uint32_t)(fn + 1), (uint32_t)(at == -1000 ? (int)c.nedge : at), (uint32_t)weight, 0u};
        c.f_rec.insert(c.f_rec.end(), rec, rec + 4);
        for (const auto &x : m) { c.m_rec.push_back(x[0]); c.m_rec.push_back(x[1]); }
        c.nedge = (int64_t)c.m_rec.size() / 2;
        c.nfactor++;
    }
    std::string plan(int sample_evidence, BpPlan &p) const { return bp_plan(c, sample_evidence, NSK_BP_MAX_MEMBERS, NSK_BP_MAX_TABLE, 16, p); }
};

static bool counts(const nsk_bp_info &i, int64_t nfactor, int64_t nedges, int64_t ntable, int64_t nmsg, int64_t nfree, int64_t nisolated,
                   int64_t nclamped, int64_t nbelief, int64_t max_table) {
    return i.nfactor == nfactor && i.nedges == nedges && i.ntable == ntable && i.nmsg == nmsg && i.nfree == nfree && i.nisolated == nisolated &&
           i.nclamped == nclamped && i.nbelief == nbelief && i.max_table == max_table && i.device_bytes == 0;
}

// ids 0 .. 7 of cardinality 2 3 2 3 2 2 2 2; 1 and 5 are evidence, 4 is in no factor, 7 has no position
static void the_structure() {
    Graph g({2, 3, 2, 3, 2, 2, 2, 2}, {0, 1, 0, 0, 0, 4, 0}, 7);
    g.factor(2, 2, 0, {{0, 1}, {0, 0}});            // names id 0 twice
    g.factor(2, 2, 1, {{1, 2}, {3, 1}});            // evidence and free
    g.factor(-1, 2, 0, {});                         // no function: no member is read, whatever the arity says
    g.factor(2, 3, 1, {{2, 0}, {7, 1}, {6, 1}});    // the middle member is clamped either way
    g.factor(2, 2, 0, {{5, 1}, {0, 0}});            // evidence first
    const I32 mrec = {0, 1, 0, 0, 0, 2, 1, 1, 0, 0, 1, 1, 2, 1, 0, 1, 1, 0};
    const I64 pm_off = {0, 2, 4, 4, 7, 9}, b_off = {0, 2, 5, 7, 10, 12, 14, 16, 18};
    const I32 slot_off = {0, 1, 3, 3, 6, 8};
    BpPlan p;
    {   // the evidence clamped
        assert(g.plan(0, p).empty());
        assert((p.state == std::vector<uint8_t>{2, 1, 2, 2, 2, 1, 2, 1}));
        assert(p.pm_off == pm_off && p.mrec == mrec && p.slot_off == slot_off && p.b_off == b_off);
        assert((p.slot_rec == I32{0, 1, 1, 0, 3, 1, 2, 1, 7, 0, 6, 1, 5, 0, 0, 1}));
        assert((p.tab_off == I64{0, 2, 5, 6, 10, 12}));                 // 2, 3 (the free member alone), 1, 4, 2
        assert((p.edge_off == I32{0, 1, 2, 2, 4, 5}));
        assert((p.e_fac == I32{0, 1, 3, 3, 4}) && (p.e_var == I32{0, 3, 2, 6, 0}));
        assert((p.msg_off == I64{0, 2, 5, 7, 9, 11}));
        assert((p.v_list == I32{0, 2, 6, 3}) && p.nvbin == 3 && !p.big);   // id 4 has a belief and no entry
        assert((p.v_eoff == I32{0, 2, 3, 4, 5}) && (p.v_edges == I32{0, 4, 2, 3, 1}));
        assert(counts(p.info, 5, 5, 12, 11, 5, 1, 3, 18, 4));
    }
    {   // the evidence free: id 7 alone stays clamped
        assert(g.plan(1, p).empty());
        assert((p.state == std::vector<uint8_t>{2, 2, 2, 2, 2, 2, 2, 1}));
        assert(p.pm_off == pm_off && p.mrec == mrec && p.slot_off == slot_off && p.b_off == b_off);
        assert((p.slot_rec == I32{0, 1, 1, 1, 3, 1, 2, 1, 7, 0, 6, 1, 5, 1, 0, 1}));
        assert((p.tab_off == I64{0, 2, 11, 12, 16, 20}));
        assert((p.edge_off == I32{0, 1, 3, 3, 5, 7}));
        assert((p.e_fac == I32{0, 1, 1, 3, 3, 4, 4}) && (p.e_var == I32{0, 1, 3, 2, 6, 5, 0}));
        assert((p.msg_off == I64{0, 2, 5, 8, 10, 12, 14, 16}));
        assert((p.v_list == I32{0, 2, 5, 6, 1, 3}) && p.nvbin == 4 && !p.big);
        assert((p.v_eoff == I32{0, 2, 3, 4, 5, 6, 7}) && (p.v_edges == I32{0, 6, 3, 5, 4, 1, 2}));
        assert(counts(p.info, 5, 7, 20, 16, 7, 1, 1, 18, 9));
    }
}

// free variables of cardinality 3, 2, NSK_ZLOCAL (then one more), 2 and NSK_ZLOCAL, a unary factor each, and an isolated
// one of cardinality 40
static void the_cardinalities() {
    for (int32_t third : {16, 17}) {
        Graph g({3, 2, third, 2, 16, 40}, {0, 0, 0, 0, 0, 0}, 6);
        for (int32_t v = 0; v < 5; v++) g.factor(2, 1, v & 1, {{v, 1}});
        BpPlan p;
        assert(g.plan(0, p).empty());
        assert((p.v_list == I32{1, 3, 0, 2, 4}) && p.nvbin == 2);
        assert((p.v_eoff == I32{0, 1, 2, 3, 4, 5}) && (p.v_edges == I32{1, 3, 0, 2, 4}));
        assert((p.e_fac == I32{0, 1, 2, 3, 4}) && (p.e_var == I32{0, 1, 2, 3, 4}) && (p.edge_off == I32{0, 1, 2, 3, 4, 5}));
        assert((p.msg_off == I64{0, 3, 5, 5 + third, 7 + third, 23 + third}) && p.tab_off == p.msg_off);
        assert((p.b_off == I64{0, 3, 5, 5 + third, 7 + third, 23 + third, 63 + third}));
        assert(p.big == (third == 17));             // (the isolated variable's 40 values set nothing)
        assert(counts(p.info, 5, 5, 23 + third, 23 + third, 6, 1, 0, 63 + third, third));
    }
}

// factor 0 (unary on id 0) is fine, factor 1 offends: the text names factor 1.  ok: the nearest graph that is accepted.
static std::string refusal(const Graph &base, int fn, int arity, int weight, const Members &m, int at = -1000, int sample_evidence = 0) {
    Graph g = base;
    g.factor(2, 1, 0, {{0, 1}});
    g.factor(fn, arity, weight, m, at);
    BpPlan p;
    return g.plan(sample_evidence, p);
}

static void the_refusals() {
    const std::string F1 = "nsk_bp_setup: factor 1 ";
    Graph b({2, 2, 0}, {0, 0, 0}, 3);               // id 2 has no value to take
    b.c.logtab = {0.0, 0.5, 1.0};
    assert(refusal(b, 2, 2, 1, {{0, 1}, {1, 1}}).empty());
    const std::string unknown = F1 + "has an unknown function or a weight outside the table";
    assert(refusal(b, 5, 1, 0, {{1, 1}}) == unknown && refusal(b, 31, 1, 0, {{1, 1}}) == unknown);
    assert(refusal(b, 2, 1, 2, {{1, 1}}) == unknown && refusal(b, 2, 1, -1, {{1, 1}}) == unknown);
    assert(refusal(b, 30, 1, 0, {{1, 1}}) == F1 + "is UFO, which reads its members by value: belief propagation has no table for it");
    const std::string head = F1 + "reads its head at the literal edge index (function 13, 16 or 17 without NSK_FLAG_HEAD_BY_VID): it has no single energy";
    for (int fn : {13, 16, 17}) assert(refusal(b, fn, 2, 0, {{0, 1}, {1, 1}}) == head);
    {
        Graph v = b;
        v.c.flags = NSK_FLAG_HEAD_BY_VID;
        for (int fn : {13, 16, 17}) assert(refusal(v, fn, 2, 0, {{0, 1}, {1, 1}}).empty());
    }
    assert(refusal(b, 8, 3, 0, {{0, 1}, {1, 1}, {0, 1}}) == F1 + "(RATIO) has more members than the logarithm table");
    assert(refusal(b, 8, 2, 0, {{0, 1}, {1, 1}}).empty());
    const std::string outside = F1 + "has member positions outside the edge array";
    assert(refusal(b, 2, 3, 0, {{0, 1}, {1, 1}}) == outside);           // the arity runs past the end
    assert(refusal(b, 2, 1, 0, {{1, 1}}, -1) == outside && refusal(b, 2, 1, 0, {{1, 1}}, 2) == outside);
    assert(refusal(b, 21, 1, 0, {{1, 1}}) == outside);                  // a function that reads two positions whatever the arity
    assert(refusal(b, 2, 1, 0, {{1, 1}}, 0).empty());                   // (factor 0's own position)
    const std::string member = F1 + "has a member outside the variables";
    assert(refusal(b, 2, 1, 0, {{3, 1}}) == member && refusal(b, 2, 1, 0, {{-1, 1}}) == member);
    {
        Graph v = b;                                // internal id 3 exists and belongs to no variable
        v.c.nid = 4;
        v.c.v_card_i.push_back(0);
        assert(refusal(v, 2, 1, 0, {{3, 1}}) == member);
    }
    assert(refusal(b, 2, 2, 0, {{1, 1}, {2, 1}}) == F1 + "has a free member of cardinality below 1");
    // 18 binary variables, all evidence: clamped they cost no table entry, free they double it
    Graph w(I32(18, 2), I32(18, 1), 18);
    Members m;
    for (int32_t v = 1; v <= 17; v++) m.push_back({v, 1});
    assert(refusal(w, 2, 17, 0, m) == F1 + "has more than NSK_BP_MAX_MEMBERS = 16 distinct members");
    m.pop_back();
    m.push_back({1, 0});                            // 17 positions, 16 distinct members
    assert(refusal(w, 2, 17, 0, m).empty());
    m.resize(13);
    assert(refusal(w, 2, 13, 0, m, -1000, 1) == F1 + "has a table of more than NSK_BP_MAX_TABLE = 4096 entries over its free members");
    m.resize(12);
    {
        Graph g = w;
        g.factor(2, 1, 0, {{0, 1}});
        g.factor(2, 12, 0, m);
        BpPlan p;
        assert(g.plan(1, p).empty() && (p.tab_off == I64{0, 2, 4098}) && p.info.max_table == 4096 && p.info.nedges == 13);
    }
    {   // a variable without an internal id
        Graph g = b;
        g.c.iid[1] = 3;
        BpPlan p;
        assert(g.plan(0, p) == "nsk_bp_setup: a variable without an internal id");
    }
}

int main() {
    the_structure();
    the_cardinalities();
    the_refusals();
    std::puts("bp plan ok");
    return 0;
}
"""


def test_the_bp_plan_under_sanitizers(tmp_path):
    cxx, san = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    src, exe = tmp_path / "bp_plan_main.cpp", tmp_path / "bp_plan_main"
    src.write_text(PROGRAM)
    cmd = cxx + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread"] + san + ["-I", CSRC, str(src), "-o", str(exe)]
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:       # (a compiler without these switches)
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr)
    assert "bp plan ok" in run.stdout
