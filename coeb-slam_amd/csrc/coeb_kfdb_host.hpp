// coeb_kfdb_host.hpp -- the host half of the keyframe database (coeb_kfdb.hip): the arithmetic of
// KeyFrameDatabase::DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:199-253) that needs no
// device, kept apart so that it is tested without one.  Host code only (no HIP).
#pragma once
#include <stdint.h>

// int minCommonWords = maxCommonWords * 0.8f  (:235): a float multiply, truncated
int kfdb_min_common(int max_common);

// lKFsSharingWords (:207-222): the slots with common > 0 in the order the inverted file meets them
// first -- ascending smallest common word, then insertion sequence.  first_word[slot] is read only
// where common[slot] > 0.  order holds nslots entries; returns the list's length.
int kfdb_sharing_order(const int32_t* common, const int32_t* first_word, const int64_t* seq, int nslots, int32_t* order);

// bow_word strictly ascending and non-negative
bool kfdb_words_ascending(const int32_t* word, int nw);
