// TEST INFRASTRUCTURE ONLY.  The handful of Win32 names the reference's transfer.cpp uses (transfer.cpp:46,62,65-69),
// so that it compiles unchanged off Windows.  "Threads" run at once in the caller: each one reads and writes only the
// pixels of its own rows start..end (transfer.cpp:15-40), so running them one after the other computes what the
// threads compute.  The wait and the close ignore their handles: the reference passes all 16 slots of its array, the
// ones it never filled included.
#ifndef STITCH_ORACLE_WIN32_SHIM_H
#define STITCH_ORACLE_WIN32_SHIM_H
typedef void *HANDLE;
typedef unsigned long DWORD;
typedef DWORD (*LPTHREAD_START_ROUTINE)(void *);
#define TRUE 1
#define INFINITE 0xFFFFFFFFul
static inline HANDLE CreateThread(void *, unsigned long, LPTHREAD_START_ROUTINE f, void *arg, DWORD, void *) { f(arg); return (HANDLE)0; }
static inline DWORD WaitForMultipleObjects(DWORD, const HANDLE *, int, DWORD) { return 0; }
static inline int CloseHandle(HANDLE) { return 1; }
#endif
