// The lock-free union-find of f3d_label_components (include/f3d.h): find, union and flatten over an array of 32-bit
// parents, written against one primitive set so that the same text runs in the kernels and, with std::atomic behind it, in a host
// program under a sanitizer (tests/components_uf_main.cpp).  Nothing else is included here.
//
// P is the parent array as the caller sees it and supplies
//   unsigned load(unsigned i)                 a read of parent[i] that may be stale: any value parent[i] held at some earlier time
//   unsigned fetch_min(unsigned i, unsigned v) parent[i] = min(parent[i], v) atomically for the whole device; returns the value before
//   void     store(unsigned i, unsigned v)     a plain write (flatten only: a pass of its own, in which nothing but flatten runs)
//
// Invariants.  parent[i] <= i always, and a parent only ever decreases: the only writes are fetch_min and flatten's store of a root,
// which is no larger than what it replaces.  So every loop below walks a strictly decreasing index and ends by the lane's own progress;
// no lane waits for another.
//
// What correctness rests on.  Loads are hints: a stale parent is a former parent, and a walk over former parents ends at a voxel that
// was a root at some time.  Whether it still is one is decided by fetch_min alone: its return value is the true parent at the moment of
// the operation.  If that value is the index itself, the root has just been hung below the smaller one and the two sets are one.  If
// not, the voxel had already been given the parent `old`; its parent is now min(old, smaller) and the link that may have been taken
// away, to `old`, is owed again: the union goes on with (old, smaller), both strictly below where it stood.
#ifndef F3D_UNION_FIND_H_
#define F3D_UNION_FIND_H_

#ifndef F3D_UF_FN
#define F3D_UF_FN inline
#endif

namespace f3d_uf {

constexpr unsigned kBackground = 0xffffffffu;  // the parent of a voxel that is not foreground

// the end of the chain of (possibly stale) parents from i: a voxel that was a root when it was read
template <typename P>
F3D_UF_FN unsigned find(P& parent, unsigned i)
{
  for (;;) {
    const unsigned p = parent.load(i);
    if (p >= i) return i;  // p == i; never above (and a background voxel is never walked)
    i = p;                 // strictly smaller
  }
}

// joins the sets of a and b (both foreground)
template <typename P>
F3D_UF_FN void unite(P& parent, unsigned a, unsigned b)
{
  for (;;) {
    a = find(parent, a);
    b = find(parent, b);
    if (a == b) return;
    const unsigned larger = a > b ? a : b, smaller = a > b ? b : a;
    const unsigned old = parent.fetch_min(larger, smaller);
    if (old == larger) return;  // it was a root and now hangs below `smaller`
    a = old;                    // it had the parent old < larger already: (old, smaller) is still owed
    b = smaller;
  }
}

// the root of i, stored as its parent.  Runs in a pass after every unite has returned: the forest no longer changes but for these stores,
// which replace a parent by the root of the same tree.
template <typename P>
F3D_UF_FN unsigned flatten(P& parent, unsigned i)
{
  const unsigned root = find(parent, i);
  if (root != i) parent.store(i, root);
  return root;
}

}  // namespace f3d_uf
#endif  // F3D_UNION_FIND_H_
