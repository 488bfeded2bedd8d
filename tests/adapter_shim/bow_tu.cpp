// Compile check of the bag-of-words adapters (adapter/BoW_coeb.h and ORBmatcher_coeb.h's
// SearchByBoW) against reference-shaped types and DBoW2-shaped containers: bow_exec.cpp without
// its main, so the templates are instantiated (tests/test_adapter_bow.py, no GPU, no library).
#define main bow_exec_main
#include "bow_exec.cpp"
