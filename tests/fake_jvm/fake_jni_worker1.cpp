// Driver for the seeding entries of the JNI shim (loadPacJNI + loadFmiJNI, then worker1FlatJNI) over the fake JNIEnv of fake_jni.cpp,
// which is compiled into this library as it is: the same tables, arrays and exception state as the other drivers use.
#include "fake_jni.cpp"

extern "C" {

// out receives the returned long[] (n counts, then 8 longs per region); *out_n its length.
// returns 0 on success, 1 if the shim left a Java exception pending (text in err), -1 on harness failure
int fake_jvm_worker1(const char* lib, int partition, const uint8_t* pac, int64_t l_pac, int64_t primary, const int64_t l2[5], int64_t seq_len,
                     const int32_t* bwt, int64_t bwt_size, int32_t sa_intv, const int64_t* sa, int64_t n_sa, const int32_t opt_ints[10],
                     const int8_t mat[25], const int32_t seed_ints[5], const double seed_floats[4], int32_t flags, int n_reads,
                     const int32_t* read_len, const uint8_t* reads, int64_t reads_bytes, int64_t* out, int64_t out_cap, int64_t* out_n,
                     char* err, int errcap) {
  Jvm vm;
  g_vm = &vm;
  vm.partition = partition;
  Env e;
  FObj* self = vm.alloc("cs/ucla/edu/bwaspark/jni/SWExtendFPGAJNI");
  if (pac) {
    typedef jint (*LoadFn)(JNIEnv*, jobject, jbyteArray, jlong);
    LoadFn load = (LoadFn)load_symbol(lib, "Java_cs_ucla_edu_bwaspark_jni_MateSWJNI_loadPacJNI", err, (size_t)errcap);
    if (!load) return -1;
    load(&e.env, J(vm.alloc("cs/ucla/edu/bwaspark/jni/MateSWJNI")), (jbyteArray)J(byte_array(pac, (size_t)((l_pac + 3) / 4))), (jlong)l_pac);
    if (vm.pending) { snprintf(err, (size_t)errcap, "%s", vm.pending_msg.c_str()); return 1; }
  }
  if (bwt) {
    typedef jint (*FmiFn)(JNIEnv*, jobject, jlong, jlongArray, jlong, jintArray, jint, jlongArray);
    FmiFn fmi = (FmiFn)load_symbol(lib, "Java_cs_ucla_edu_bwaspark_jni_SWExtendFPGAJNI_loadFmiJNI", err, (size_t)errcap);
    if (!fmi) return -1;
    const jint nd = fmi(&e.env, J(self), (jlong)primary, (jlongArray)J(long_array(l2, 5)), (jlong)seq_len,
                        (jintArray)J(int_array(bwt, (size_t)bwt_size)), (jint)sa_intv, (jlongArray)J(long_array(sa, (size_t)n_sa)));
    if (vm.pending) { snprintf(err, (size_t)errcap, "%s", vm.pending_msg.c_str()); return 1; }
    if (nd < 1) { snprintf(err, (size_t)errcap, "loadFmiJNI loaded no device"); return -1; }
  }
  typedef jlongArray (*Fn)(JNIEnv*, jobject, jintArray, jbyteArray, jintArray, jdoubleArray, jint, jintArray, jbyteArray);
  Fn fn = (Fn)load_symbol(lib, "Java_cs_ucla_edu_bwaspark_jni_SWExtendFPGAJNI_worker1FlatJNI", err, (size_t)errcap);
  if (!fn) return -1;
  jlongArray r = fn(&e.env, J(self), (jintArray)J(int_array(opt_ints, 10)), (jbyteArray)J(byte_array(reinterpret_cast<const uint8_t*>(mat), 25)),
                    (jintArray)J(int_array(seed_ints, 5)), (jdoubleArray)J(double_array(seed_floats, 4)), (jint)flags,
                    (jintArray)J(int_array(read_len, (size_t)n_reads)), (jbyteArray)J(byte_array(reads, (size_t)reads_bytes)));
  if (vm.pending) { snprintf(err, (size_t)errcap, "%s", vm.pending_msg.c_str()); return 1; }
  if (!r) { snprintf(err, (size_t)errcap, "null result"); return -1; }
  *out_n = (int64_t)O(r)->la.size();
  if (*out_n > out_cap) { snprintf(err, (size_t)errcap, "out_cap too small"); return -1; }
  memcpy(out, O(r)->la.data(), 8 * (size_t)*out_n);
  return 0;
}

}  // extern "C"
