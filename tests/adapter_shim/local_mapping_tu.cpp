// Compile check of the LocalMapping adapter (adapter/LocalMapping_coeb.h) against reference-shaped
// types: local_mapping_exec.cpp without its main, so the templates are instantiated
// (tests/test_adapter_tri.py, no GPU, no library).
#define main local_mapping_exec_main
#include "local_mapping_exec.cpp"
