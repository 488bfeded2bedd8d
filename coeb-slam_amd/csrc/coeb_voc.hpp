// coeb_voc.hpp -- the bag-of-words vocabulary behind the C-ABI's coeb_voc handle (host code, no HIP).
//
// A DBoW2 TemplatedVocabulary<ORB> is a k-ary tree of 32-byte descriptors with a weight per leaf
// (word).  Node ids are the file's: 0 is the root, line i of ORBvoc.txt defines node i.  The
// tables below are the form k_bow_transform walks (coeb_bow.hip): nodes renumbered so the
// children of every node are contiguous and in their original order ("slots"; slot 0 is the
// root), one 16-byte record and one 32-byte descriptor per slot.
#pragma once
#include <stdint.h>
#include <vector>

struct VocRec {            // one slot
    int32_t child_first;   // slot of the first child
    int32_t child_count;   // 0: a leaf
    int32_t word;          // word id of a leaf, -1 for inner nodes
    uint32_t id_flag;      // node id | kVocPositive when the leaf's weight is > 0
};
constexpr uint32_t kVocPositive = 0x80000000u;

struct coeb_voc {
    int k = 0, L = 0, scoring = 0, weighting = 0;
    int nnodes = 0;                    // with the root
    int nwords = 0;
    std::vector<VocRec> rec;           // [nnodes] by slot
    std::vector<uint8_t> desc;         // [nnodes][32] by slot (the root's is zero)
    std::vector<int32_t> slot_of;      // [nnodes] node id -> slot
    std::vector<double> word_weight;   // [nwords]
    std::vector<int32_t> word_node;    // [nwords] node id of the word
};
